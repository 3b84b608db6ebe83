"""Run-time AIRs on the GPU (csrc/air_program.hip: the interpreter's K5 and trace-checker kernels; bp_stark_prove_trace):
K5 of a registered transcription against the built-in kernel word for word, bp_stark_prove_trace against
bp_stark_prove_air byte for byte, whole proofs under a registered id, AIR 3's transcription through the device checker
and the verifier, a Fibonacci-style table that is nobody's built-in, and seeded random programs (tests/air_program_random.py: degrees 1 to
9, up to 64 registers, 40 units, every operation and kind) whose only reference is the builder's evaluate() over Python
integers: the device checker, bp_quotient_eval against a fold written here, whole proofs.  Everything is exact.  CPU
side: tests/test_air_program.py."""
import numpy as np
import pytest

import air_program_cases as cases
import air_program_random as rnd
from air_program_cases import P
from util import to_dev, to_host

pytestmark = pytest.mark.gpu

PROGRAM = {3: cases.memory_program, 4: cases.arithmetic_program, 7: cases.arithmetic_mul_program}
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
    with bpg.ops.tuned(assume_loaded=loaded):
        want = bpg.ops.quotient_eval(cfg, trace, aux, None, ctl, alphas, air_id=air_id)
        got = bpg.ops.quotient_eval(cfg, trace, aux, None, ctl, alphas, air_id=reg)
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
    trace = bpg.ops.air_trace(air_id, log_n, seed=SEED + log_n)
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
    trace = bpg.ops.air_trace(air_id, log_n, seed=SEED + log_n)
    with bpg.ops.tuned(assume_loaded=loaded):
        want = bpg.ops.stark_prove_trace(air_id, cfg, trace)
        got = bpg.ops.stark_prove_trace(reg, cfg, trace)
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
    trace = bpg.ops.air_trace(air_id, 5, seed=SEED)
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
    from builtin_airs import memory
    reg = cases.register(cases.memory_program())
    log = memory.random_log(64, 11, n_addr=6)
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


# ---------------------------------------------------------------------------------------------- 12. random programs

HEIGHTS = [(name, log_n) for name in rnd.CASES for log_n in (5, 8, 12)] + [(name, 15) for name in rnd.CASES if rnd.case(name).tall]
HEIGHT_IDS = ["%s@%d" % h for h in HEIGHTS]
assert sorted(rnd.case(name).deg_pow for name, log_n in HEIGHTS if log_n == 15) == [1, 3]   # one tall case of each deg_pow


def reported(r):
    return [(v.row, v.constraint, v.family, v.kind, v.value) for v in r.violations]


def device_witness(name, log_n):
    trace, consts, pub = rnd.witness(name, log_n)
    return trace, consts, pub, to_dev(trace.copy()), to_dev(consts.copy())      # (the cached arrays are read-only)


@pytest.mark.parametrize("name,log_n", HEIGHTS, ids=HEIGHT_IDS)
def test_device_checker_on_a_random_program(bpg, name, log_n):
    """The constructed witness (wrong slack cells wherever a kind is switched off) is clean; with five random cells, a
    first-row slack cell in row 0 and a last-row one in row n - 1 changed, the device reports what the host pass
    reports, and its first 16 violations are evaluate()'s.  Spread over grid.y and in one pass."""
    c = rnd.case(name)
    reg = bpg.ops.air_register(c.words)
    trace, consts, pub, t, cd = device_witness(name, log_n)
    n = 1 << log_n
    rng = np.random.default_rng([0x900, c.kw["seed"], log_n])
    bad = trace.copy()
    cells = [(int(rng.integers(0, n)), int(rng.integers(0, c.b.n_cols))) for _ in range(5)]
    cells += [rnd.active_cell(c, rnd.FIRST_ROW, n, rng), rnd.active_cell(c, rnd.LAST_ROW, n, rng)]
    for row, col in cells:
        bad[col, row] = (int(bad[col, row]) + 1 + int(rng.integers(0, 3))) % P
    host = bpg.ops.check_air_trace_host(reg, bad, consts=consts, pub=pub, max_rows=64, max_viol=4096)
    key = lambda r: (r.n_violated_rows, r.rows, r.n_violations, reported(r))
    assert host.n_violated_rows >= 2 and host.rows[0] == 0 and host.rows[-1] == n - 1
    assert reported(host)[:16] == rnd.violations(c.b, bad, consts, pub, host.rows)[:16]
    for loaded in (0, 1):
        with bpg.ops.tuned(assume_loaded=loaded):
            r = bpg.ops.check_air_trace(reg, t, consts=cd, pub=pub)
            dev = bpg.ops.check_air_trace(reg, to_dev(bad), consts=cd, pub=pub, max_rows=64, max_viol=4096)
        assert r.ok and r.rows == [] and r.violations == [], (loaded, r)
        assert key(dev) == key(host), loaded


def python_quotient(c, log_n, loc, nxt, cst, aux, aux_nxt, alphas, pos):
    """Both quotient words at coset-major position pos = t n + m, over Python integers: the point
    x = 7 w_{n 2^r}^(t + 2^r m); constraint i of kind k times its selector -- 1, x - g^-1, L_0(x) = Z_H(x) / (n (x - 1)),
    L_{n-1}(x) = Z_H(x) / (n (g x - 1)), g = w_n -- weighed with alpha_j^(T - 1 - i), T = the program's constraints + the
    two of the constant running product z (transition z - z', last row z - 1: AIRS.md section 3 with no filter, term = 1),
    the sum divided by Z_H(x) = x^n - 1.  bp_quotient_eval takes no public inputs: pub(j) reads zero there."""
    n, r = 1 << log_n, c.rate_bits
    t, m = pos >> log_n, pos & (n - 1)
    inv = lambda v: pow(v % P, P - 2, P)
    x = 7 * pow(pow(7, (P - 1) >> (log_n + r), P), t + (m << r), P) % P
    g = pow(7, (P - 1) >> log_n, P)
    zh = (pow(x, n, P) - 1) % P
    sel = [1, (x - inv(g)) % P, zh * inv(n * (x - 1)) % P, zh * inv(n * (g * x - 1)) % P]
    vals = c.b.evaluate(loc, nxt, cst, (0, 0, 0, 0), x)
    terms = [(i, f[2], vals[i]) for f in c.b.families for i in range(f[0], f[0] + f[1])]
    T = c.n_constraints + 2
    terms += [(T - 2, rnd.TRANSITION, (aux - aux_nxt) % P), (T - 1, rnd.LAST_ROW, (aux - 1) % P)]
    return [sum(pow(a, T - 1 - i, P) * sel[kind] * v for i, kind, v in terms) * inv(zh) % P for a in alphas]


@pytest.mark.parametrize("name,log_n", HEIGHTS, ids=HEIGHT_IDS)
def test_quotient_eval_of_a_random_program_equals_the_fold_over_python_integers(bpg, name, log_n):
    """K5 without the verifier: the LDE of the witness and the constants (ops.lde_batch, pinned to the oracle elsewhere),
    an auxiliary LDE of all ones (the constant running product: its two constraints vanish identically), and both
    quotient words recomputed by python_quotient at 48 positions: every coset, m in {0, 1, n - 2, n - 1} (the next row
    wraps inside the coset) and random m.  On the coset a kind that is 'switched off' is not: the wrong slack cells of
    the witness enter through the selectors, and the quotient of a valid witness is still a polynomial -- which is why
    the values are compared with a fold and not with zero.  Spread and one-pass launches give the same words."""
    import torch
    c = rnd.case(name)
    reg = bpg.ops.air_register(c.words)
    trace, consts, pub, t, cd = device_witness(name, log_n)
    n, r = 1 << log_n, c.rate_bits
    rows = n << r
    _, lde = bpg.ops.lde_batch(t, r)
    _, clde = bpg.ops.lde_batch(cd, r)
    aux = torch.ones((1, rows), dtype=torch.int64, device="cuda")
    rng = np.random.default_rng([0x901, c.kw["seed"], log_n])
    ctl = [int(v) for v in rng.integers(2, P, size=4, dtype=np.uint64)]
    alphas = [int(v) for v in rng.integers(2, P, size=2, dtype=np.uint64)]
    cfg = bpg.ops.stark_cfg(log_n, c.b.n_cols, n_const=c.b.n_const, deg_pow=c.deg_pow, rate_bits=r)
    got = []
    for loaded in (0, 1):
        with bpg.ops.tuned(assume_loaded=loaded):
            got.append(bpg.ops.quotient_eval(cfg, lde, aux, clde, ctl, alphas, air_id=reg))
    assert got[0].shape == got[1].shape == (2, rows) and bool((got[0] == got[1]).all()), "spread != one-pass"
    assert bool((got[0] != 0).any())
    ms = [0, 1, n - 2, n - 1]
    pos = [tt * n + m for tt in range(1 << r) for m in ms]
    pos += [int(v) for v in rng.integers(0, rows, size=48 - len(pos))]
    assert len(pos) == 48 and {p >> log_n for p in pos} == set(range(1 << r))
    nxt = [(p >> log_n) * n + ((p & (n - 1)) + 1) % n for p in pos]
    idx = torch.tensor(pos + nxt, dtype=torch.int64, device="cuda")
    L, CL, Q = to_host(lde[:, idx].contiguous()), to_host(clde[:, idx].contiguous()), to_host(got[0][:, idx[:48]].contiguous())
    for k, p in enumerate(pos):
        want = python_quotient(c, log_n, L[:, k], L[:, 48 + k], CL[:, k], 1, 1, alphas, p)
        assert [int(Q[0, k]), int(Q[1, k])] == want, (name, log_n, "position", p, "coset", p >> log_n, "m", p & (n - 1))


PROOF_COST = {5: (6, 6), 8: (20, 10), 12: (84, 16), 15: (84, 16)}


@pytest.mark.parametrize("name,log_n", HEIGHTS, ids=HEIGHT_IDS)
def test_a_random_program_proves_and_verifies(bpg, name, log_n):
    """bp_stark_prove_trace of the constructed witness verifies; a flipped bit, each public input the program reads
    changed, a wrong constants commitment and a proof made from a witness with one ACTIVE slack cell changed are each
    rejected, the last at the constraint check at zeta."""
    c = rnd.case(name)
    reg = bpg.ops.air_register(c.words)
    trace, consts, pub, t, cd = device_witness(name, log_n)
    n = 1 << log_n
    nq, pb = PROOF_COST[log_n]
    cfg = cases.cfg_for(reg, log_n, num_queries=nq, pow_bits=pb)
    assert (cfg.n_cols, cfg.n_const, cfg.deg_pow, cfg.rate_bits) == (c.b.n_cols, c.b.n_const, c.deg_pow, c.rate_bits)
    cap = constants_cap(bpg, cd, log_n, rate_bits=c.rate_bits)
    rng = np.random.default_rng([0x902, c.kw["seed"], log_n])
    for loaded in ((0, 1) if log_n <= 8 else ((rnd.CASES.index(name) + log_n) % 2,)):
        with bpg.ops.tuned(assume_loaded=loaded):
            proof = bpg.ops.stark_prove_trace(reg, cfg, t, consts=cd, pub=pub)
        assert int(proof[14]) == reg
        assert cases.verify(reg, cfg, proof, cap, pub) == 0, (loaded, bpg.lib().bp_last_error())
    flipped = proof.copy()
    flipped[proof.size // 2 + int(rng.integers(0, 8))] ^= np.uint64(1 << int(rng.integers(0, 32)))
    assert cases.verify(reg, cfg, flipped, cap, pub) == -5
    for j in range(c.b.n_public):
        wrong = list(pub)
        wrong[j] = (wrong[j] + 1) % P
        assert cases.verify(reg, cfg, proof, cap, wrong) == -5, j
    other = consts.copy()
    other[c.b.n_const - 1, int(rng.integers(0, n))] ^= np.uint64(1)
    assert cases.verify(reg, cfg, proof, constants_cap(bpg, to_dev(other), log_n, rate_bits=c.rate_bits), pub) == -5
    kind = rnd.KINDS[int(rng.integers(0, 4))]
    row, col = rnd.active_cell(c, kind, n, rng)
    bad = trace.copy()
    bad[col, row] = (int(bad[col, row]) + 1) % P
    assert not bpg.ops.check_air_trace_host(reg, bad, consts=consts, pub=pub).ok
    assert cases.verify(reg, cfg, bpg.ops.stark_prove_trace(reg, cfg, to_dev(bad), consts=cd, pub=pub), cap, pub) == -5, (kind, row, col)
    assert b"constraint check at zeta" in bpg.lib().bp_last_error()


@pytest.mark.parametrize("at_cap,above", [("deg3-u5", "first-row-deg3"), ("deg9-u5", "first-row-deg9")])
def test_first_row_and_last_row_families_at_their_degree_cap_verify_and_above_it_are_refused(bpg, at_cap, above):
    """The degree rule of first-row and last-row families (include/bpg.h, AIRS.md section 1).  The programs `above`
    (degree 3 with cubic first-row and last-row families; degree 9 with families of degree 9) used to register; the
    quotient of such a family has degree (d + 1)(n - 1) - n and does not fit the 2^rate_bits n coefficients of a proof
    (tests/test_air_program.py computes it over Python integers: 92 against 64, 278 against 256 at 2^5 rows), so the
    rule refuses them at registration.  Here: families AT the cap, degree 2 in a degree-3 program and 8 in a degree-9
    one, prove and verify at 2^5 rows, where (d + 1)(n - 1) - n is closest to the bound relative to n."""
    from proof_protocol_decoder_amd._lib import BpgError
    with pytest.raises(BpgError, match="-row family of degree"):
        bpg.ops.air_register(rnd.case(above).words)
    c = rnd.case(at_cap)
    cap = rnd.boundary_degree_cap(c.degree)
    assert {f[2] for f in c.b.families if f[2] >= 2 and f[3] == cap} == {rnd.FIRST_ROW, rnd.LAST_ROW}
    reg = bpg.ops.air_register(c.words)
    trace, consts, pub, t, cd = device_witness(at_cap, 5)
    cfg = cases.cfg_for(reg, 5, num_queries=6, pow_bits=6)
    proof = bpg.ops.stark_prove_trace(reg, cfg, t, consts=cd, pub=pub)
    assert cases.verify(reg, cfg, proof, constants_cap(bpg, cd, 5, rate_bits=c.rate_bits), pub) == 0
