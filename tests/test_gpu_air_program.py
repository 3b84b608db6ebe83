"""Run-time AIRs on the GPU (csrc/air_program.hip: the interpreter's K5 and trace-checker kernels; bp_stark_prove_trace):
K5 of a registered transcription against the built-in kernel word for word, bp_stark_prove_trace against
bp_stark_prove_air byte for byte, whole proofs under a registered id, AIR 3's transcription through the device checker
and the verifier, and a Fibonacci-style table that is nobody's built-in.  Everything is exact.  CPU side:
tests/test_air_program.py."""
import numpy as np
import pytest

import air_program_cases as cases
from air_program_cases import P
from util import to_dev, to_host

pytestmark = pytest.mark.gpu

PROGRAM = {3: cases.memory_program, 4: cases.arithmetic_program, 7: cases.arithmetic_mul_program}
TRACE = {3: "memory_trace", 4: "arithmetic_trace", 7: "arithmetic_mul_trace"}
SEED = 0x5EED00000000A1F0


def random_lde(n_cols, rows, seed):
    """uniform words below 2^63 (canonical), the field's edge values sprinkled in, made on the device"""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    m = torch.randint(0, 2 ** 63 - 1, (n_cols, rows), dtype=torch.int64, device="cuda", generator=g)
    flat = m.view(-1)
    for k, v in enumerate([0, 1, P - 1, 0xFFFFFFFF, 1 << 32, P - (1 << 32), 0xFFFFFFFF00000000, 2]):
        flat[(k * 7919) % flat.numel()] = v - (1 << 64) if v >= 1 << 63 else v
    return m


def set_cell(t, col, row, value):
    t[col, row] = value - (1 << 64) if value >= 1 << 63 else value


def cell(t, col, row):
    return int(t[col, row].item()) & (2 ** 64 - 1)


# ---------------------------------------------------------------------------------------------- 7. K5 alone


@pytest.mark.parametrize("air_id,log_n", [(4, 10), (4, 16), (7, 9), (7, 14)])
@pytest.mark.parametrize("loaded", [0, 1], ids=["spread", "one-pass"])
def test_quotient_eval_equals_the_built_in_kernel(bpg, air_id, log_n, loaded):
    """Random LDE matrices (on the coset the 'bit' columns are arbitrary field elements): every word of the quotient
    values of the registered transcription equals the built-in quotient_air_kernel's, spread over grid.y and in one pass,
    at a height that fills the chip and at one that does not."""
    reg = cases.register(PROGRAM[air_id]())
    d = bpg.ops.air_describe(air_id)
    rows = (1 << log_n) << 1
    trace, aux = random_lde(d.n_cols, rows, 900 + log_n), random_lde(1, rows, 901 + log_n)
    rng = np.random.default_rng(902 + log_n)
    ctl = [int(v) for v in rng.integers(2, P, size=4, dtype=np.uint64)]
    alphas = [int(v) for v in rng.integers(2, P, size=2, dtype=np.uint64)]
    cfg = bpg.ops.stark_cfg(log_n, d.n_cols)
    bpg.lib().bp_tune_assume_loaded(loaded)
    try:
        want = bpg.ops.quotient_eval(cfg, trace, aux, None, ctl, alphas, air_id=air_id)
        got = bpg.ops.quotient_eval(cfg, trace, aux, None, ctl, alphas, air_id=reg)
    finally:
        bpg.lib().bp_tune_assume_loaded(-1)
    assert got.shape == want.shape == (2, rows)
    assert bool((got == want).all()), "first mismatch at %s" % (got != want).nonzero()[0].tolist()
    assert bool((want != 0).any())


# ---------------------------------------------------------------------------------------------- 8. bp_stark_prove_trace alone


@pytest.mark.parametrize("air_id,log_n,nq,pb", [(4, 5, 6, 6), (4, 12, 84, 16), (7, 5, 6, 6), (7, 10, 20, 10), (3, 9, 20, 10)])
def test_prove_trace_with_a_built_in_id_is_prove_air(bpg, air_id, log_n, nq, pb):
    """the proof from the device trace of bp_*_trace(seed) is bp_stark_prove_air(id, cfg, seed)'s, byte for byte (bytes
    the oracle pins); a column slice of a wider buffer (stride > n) gives the same"""
    import torch
    cfg = cases.cfg_for(air_id, log_n, num_queries=nq, pow_bits=pb)
    want = bpg.ops.stark_prove_air(air_id, cfg, SEED + log_n)
    trace = getattr(bpg.ops, TRACE[air_id])(log_n, seed=SEED + log_n)
    got = bpg.ops.stark_prove_trace(air_id, cfg, trace)
    assert got.shape == want.shape and (got == want).all() and int(got[14]) == air_id
    if log_n <= 9:
        wide = torch.zeros((trace.shape[0], 3 << log_n), dtype=torch.int64, device="cuda")
        wide[:, :1 << log_n] = trace
        assert (bpg.ops.stark_prove_trace(air_id, cfg, wide[:, :1 << log_n]) == want).all()


def test_prove_trace_refuses_bad_arguments(bpg):
    from proof_protocol_decoder_amd._lib import BpgError
    trace = bpg.ops.arithmetic_trace(5, seed=1)
    with pytest.raises(BpgError, match="arithmetic"):
        bpg.ops.stark_prove_trace(4, bpg.ops.stark_cfg(5, 309, n_const=1, num_queries=6, pow_bits=6), trace)
    fib = cases.register(cases.fibonacci_program())
    t, m, pub = cases.fibonacci_witness(5, 1, 2)
    cfg = cases.cfg_for(fib, 5, num_queries=6, pow_bits=6)
    with pytest.raises(BpgError, match="constant columns"):
        bpg.ops.stark_prove_trace(fib, cfg, to_dev(t), consts=None, pub=pub)
    with pytest.raises(BpgError, match="public inputs"):
        bpg.ops.stark_prove_trace(fib, cfg, to_dev(t), consts=to_dev(m), pub=None)
    with pytest.raises(BpgError, match="non-canonical"):
        bpg.ops.stark_prove_trace(fib, cfg, to_dev(t), consts=to_dev(m), pub=[P, 0, 0, 0])


# ---------------------------------------------------------------------------------------------- 9. whole proofs


@pytest.mark.parametrize("air_id,log_n,nq,pb,loaded", [(4, 5, 6, 6, 0), (4, 12, 84, 16, 1), (4, 16, 84, 16, 0),
                                                        (7, 5, 6, 6, 0), (7, 12, 84, 16, 1), (7, 14, 84, 16, 0)])
def test_a_registered_transcription_gives_the_built_ins_proof(bpg, air_id, log_n, nq, pb, loaded):
    """AIR 4 and AIR 7 have exactly the auxiliary column a registered AIR gets, and the air_id is in no transcript: the
    proof under the registered id equals the built-in's in every word but header word 14, up to the heights
    tests/test_gpu_arithmetic*_air.py prove (2^16 / 2^14 rows); it verifies under its id only."""
    reg = cases.register(PROGRAM[air_id]())
    cfg = cases.cfg_for(air_id, log_n, num_queries=nq, pow_bits=pb)
    trace = getattr(bpg.ops, TRACE[air_id])(log_n, seed=SEED + log_n)
    bpg.lib().bp_tune_assume_loaded(loaded)
    try:
        want = bpg.ops.stark_prove_trace(air_id, cfg, trace)
        got = bpg.ops.stark_prove_trace(reg, cfg, trace)
    finally:
        bpg.lib().bp_tune_assume_loaded(-1)
    assert got.shape == want.shape and int(got[14]) == reg and int(want[14]) == air_id
    diff = np.nonzero(got != want)[0]
    assert diff.tolist() == [14], diff[:10]
    assert cases.verify(reg, cfg, got) == 0
    assert cases.verify(air_id, cfg, got) == -5 and cases.verify(reg, cfg, want) == -5
    flipped = got.copy()
    flipped[got.size // 2] ^= np.uint64(1 << 21)
    assert cases.verify(reg, cfg, flipped) == -5


@pytest.mark.parametrize("air_id,col,row", [(4, 292 + 7, 11), (4, 36 + 100, 0), (7, 545 + 21 * 9 + 4, 9), (7, 1 + 6, 31)])
def test_a_corrupted_trace_yields_a_rejected_proof(bpg, air_id, col, row):
    reg = cases.register(PROGRAM[air_id]())
    cfg = cases.cfg_for(air_id, 5, num_queries=6, pow_bits=6)
    trace = getattr(bpg.ops, TRACE[air_id])(5, seed=SEED)
    assert cases.verify(reg, cfg, bpg.ops.stark_prove_trace(reg, cfg, trace)) == 0
    set_cell(trace, col, row, cell(trace, col, row) ^ 1)
    assert not bpg.ops.check_air_trace(reg, trace).ok
    assert cases.verify(reg, cfg, bpg.ops.stark_prove_trace(reg, cfg, trace)) == -5
    assert b"constraint check at zeta" in bpg.lib().bp_last_error()


# ---------------------------------------------------------------------------------------------- 10. AIR 3's transcription


@pytest.mark.parametrize("log_n,nq,pb", [(6, 6, 6), (13, 84, 16)])
def test_memory_trace_proven_through_the_registered_id_verifies(bpg, log_n, nq, pb):
    reg = cases.register(cases.memory_program())
    cfg = cases.cfg_for(reg, log_n, num_queries=nq, pow_bits=pb)
    proof = bpg.ops.stark_prove_trace(reg, cfg, bpg.ops.memory_trace(log_n, seed=SEED + log_n))
    assert int(proof[14]) == reg and cases.verify(reg, cfg, proof) == 0
    assert int(proof[4]) == 1                              # one auxiliary column (the built-in memory table has two)


def corrupt(t, k, rng):
    rows = sorted(int(x) for x in rng.choice(t.shape[1], size=k, replace=False))
    for i in rows:
        c = int(rng.integers(0, t.shape[0] - 1))          # (column 44 is the built-in's lookup filter: not the AIR's own)
        set_cell(t, c, i, (cell(t, c, i) + 1 + int(rng.integers(0, 3))) % P)
    return rows


@pytest.mark.parametrize("log_n", [6, 9, 10, 13, 17])
def test_device_checker_agrees_with_the_host_pass(bpg, log_n):
    """clean and corrupted memory traces from 2^6 to 2^17 rows (grid.y spreading does not apply to a one-unit program; the
    sizes cover one workgroup to 512): the device's rows and violations under the registered id are the host pass's, and
    the built-in id's"""
    reg = cases.register(cases.memory_program())
    rng = np.random.default_rng(0x700 + log_n)
    t = bpg.ops.memory_trace(log_n, seed=0xB0 + log_n)
    r = bpg.ops.check_air_trace(reg, t)
    assert r.ok and r.rows == [] and r.violations == []
    corrupt(t, 5, rng)
    set_cell(t, 0, 0, 1)
    set_cell(t, 3, 0, 77)                                  # a read of a non-zero value in the first row
    set_cell(t, 11, (1 << log_n) - 1, 5)                   # and a non-bit in the last row
    dev = bpg.ops.check_air_trace(reg, t, max_rows=64, max_viol=4096)
    host = bpg.ops.check_air_trace_host(reg, to_host(t), max_rows=64, max_viol=4096)
    built_in = bpg.ops.check_air_trace(3, t, max_rows=64, max_viol=4096)
    key = lambda r: (r.n_violated_rows, r.rows, r.n_violations, [(v.row, v.constraint, v.family, v.kind, v.value) for v in r.violations])
    assert dev.n_violated_rows >= 3 and 0 in dev.rows and (1 << log_n) - 1 in dev.rows
    assert key(dev) == key(host) == key(built_in)


def test_a_stale_read_is_rejected_by_the_verifier(bpg):
    from test_memory_air import random_log
    reg = cases.register(cases.memory_program())
    log = random_log(64, 11, n_addr=6)
    cfg = cases.cfg_for(reg, 6, num_queries=6, pow_bits=6)
    assert cases.verify(reg, cfg, bpg.ops.stark_prove_trace(reg, cfg, bpg.ops.memory_trace(6, inputs=to_dev(log)))) == 0
    r0 = next(i for i in range(1, 64) if log[i, 0] == 1 and log[i, 1] == log[i - 1, 1])
    log[r0, 3 + 2] ^= np.uint64(5)
    bad = bpg.ops.memory_trace(6, inputs=to_dev(log))
    r = bpg.ops.check_air_trace(reg, bad)
    assert r.rows == [r0 - 1] and {v.family for v in r.violations} == {5}
    assert cases.verify(reg, cfg, bpg.ops.stark_prove_trace(reg, cfg, bad)) == -5


# ---------------------------------------------------------------------------------------------- 11. nobody's built-in


def constants_cap(bpg, consts, log_n, rate_bits=1, cap_height=4):
    _, lde = bpg.ops.lde_batch(consts, rate_bits)
    dig = to_host(bpg.ops.merkle_commit(lde, log_n, rate_bits, cap_height))
    return np.ascontiguousarray(dig[-(1 << cap_height):].reshape(-1))


@pytest.mark.parametrize("log_n,nq,pb", [(5, 6, 6), (10, 28, 10)])
def test_a_fibonacci_table_with_constants_and_public_inputs(bpg, log_n, nq, pb):
    """cst, pub, x and the first- and last-row kinds in one program that no built-in AIR states: the witness is made
    here, checked on the device, proven and verified; a wrong public input, a wrong constants commitment and a wrong
    step are each rejected."""
    import torch
    b = cases.fibonacci_program()
    fib = cases.register(b)
    t, m, pub = cases.fibonacci_witness(log_n, 3, 5)
    trace, consts = torch.from_numpy(t.view(np.int64)).cuda(), torch.from_numpy(m.view(np.int64)).cuda()
    assert bpg.ops.check_air_trace(fib, trace, consts=consts, pub=pub).ok
    assert bpg.ops.check_air_trace_host(fib, t, consts=m, pub=pub).ok
    cfg = cases.cfg_for(fib, log_n, num_queries=nq, pow_bits=pb)
    assert (cfg.n_cols, cfg.n_const, cfg.rate_bits) == (8, 1, 1)
    proof = bpg.ops.stark_prove_trace(fib, cfg, trace, consts=consts, pub=pub)
    cap = constants_cap(bpg, consts, log_n)
    assert int(proof[14]) == fib and cases.verify(fib, cfg, proof, cap, pub) == 0
    for j in range(3):                                      # each of the three public inputs is bound
        wrong = list(pub)
        wrong[j] = (wrong[j] + 1) % P
        assert cases.verify(fib, cfg, proof, cap, wrong) == -5
        r = bpg.ops.check_air_trace(fib, trace, consts=consts, pub=wrong)
        assert r.rows == [(1 << log_n) - 1 if j == 2 else 0] and [v.kind for v in r.violations] == [3 if j == 2 else 2]
    other = m.copy()
    other[0, 7] += np.uint64(1)
    assert cases.verify(fib, cfg, proof, constants_cap(bpg, to_dev(other), log_n), pub) == -5
    # a wrong step (row 9's b), the point column and the product column: the checker names them, the verifier rejects
    for col, kinds in ((1, {0, 1}), (2, {0}), (3, {0})):
        bad = trace.clone()
        set_cell(bad, col, 9, (cell(bad, col, 9) + 1) % P)
        r = bpg.ops.check_air_trace(fib, bad, consts=consts, pub=pub)
        want = bpg.ops.check_air_trace_host(fib, to_host(bad), consts=m, pub=pub)
        assert not r.ok and r.rows == want.rows and {v.kind for v in r.violations} == kinds
        assert [(v.row, v.constraint, v.value) for v in r.violations] == [(v.row, v.constraint, v.value) for v in want.violations]
        assert cases.verify(fib, cfg, bpg.ops.stark_prove_trace(fib, cfg, bad, consts=consts, pub=pub), cap, pub) == -5
