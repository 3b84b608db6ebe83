"""The modular table on the GPU: the witness kernel (csrc/arithmetic_mod.hip) against the independent row model of
tests/arithmetic_mod_model.py word for word, then the shipped program through the run-time stack -- the device checker,
the prover and the verifier, the port's running products, and table sets in which a caller's table looks modular
operations up.  Everything is exact.  CPU side: tests/test_arithmetic_mod.py."""
import numpy as np
import pytest

import air_program_cases as cases
import air_program_port_cases as pc
import arithmetic_mod_model as model
from air_program_port_cases import LINK, cfg_of
from proof_protocol_decoder_amd import arithmetic_mod as am
from util import to_dev, to_host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def reg(bpg):
    return am.register()


def device_trace(bpg, ops):
    log_n = len(ops).bit_length() - 1
    return bpg.ops.arithmetic_mod_trace(log_n, to_dev(am.pack_inputs(ops)))


@pytest.fixture(scope="module")
def edge(bpg):
    """(operations, device trace) of the 2^5-row edge list"""
    ops = model.edge_ops()
    return ops, device_trace(bpg, ops)


def assert_equal_word_for_word(got, want):
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert not len(bad), ("first mismatches (column, row)", bad[:6].tolist(), "of", len(bad))


# 2^5: fewer rows than a workgroup; 2^7: every edge under both flags, exposed and not; 2^9: two workgroups
@pytest.mark.parametrize("which", ["edges-2^5", "edges-2^7", "random-2^9"])
def test_the_device_witness_is_the_model_and_the_checker_is_clean(bpg, reg, which):
    ops = {"edges-2^5": model.edge_ops, "edges-2^7": model.edge_ops_full, "random-2^9": lambda: model.random_ops(512, 0x9A0D)}[which]()
    t = device_trace(bpg, ops)
    assert_equal_word_for_word(to_host(t), model.trace_of(ops))
    got = bpg.ops.check_air_trace(reg, t)
    assert got.ok and got.n_violations == 0, got


def test_the_kernel_writes_every_cell_and_ignores_what_it_should(bpg):
    """a trace buffer full of ones before the call; bits 9 .. 63 of word 0 and a padding row's operands change nothing"""
    import torch
    ops = model.edge_ops()
    words = am.pack_inputs(ops)
    want = model.trace_of(ops)
    words[:, 0] |= np.uint64(0xABCDEF << 9)
    assert any(int(words[i, 1:].any()) for i, op in enumerate(ops) if op[0] not in (1, 2))   # padding rows carry junk
    out = torch.full((am.N_COLS, 32), -1, dtype=torch.int64, device="cuda")
    d_words = to_dev(words)
    assert bpg.lib().bp_arithmetic_mod_trace(d_words.data_ptr(), 5, out.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    assert_equal_word_for_word(to_host(out), want)


def test_the_edge_trace_proves_and_verifies(bpg, reg, edge):
    _, t = edge
    cfg = cases.cfg_for(reg, 5)
    assert (cfg.n_cols, cfg.rate_bits, cfg.deg_pow) == (2560, 1, 1)
    proof = bpg.ops.stark_prove_trace(reg, cfg, t)
    assert int(proof[4]) == 2 and int(proof[14]) == reg                         # two auxiliary columns: the port's products
    bpg.ops.stark_verify_air(reg, cfg, proof)
    assert cases.verify(7, cases.cfg_for(7, 5), proof) == -5                    # ... under its own id only


@pytest.mark.parametrize("entry", model.CATALOGUE, ids=[e[0] for e in model.CATALOGUE])
def test_the_proof_of_a_wrong_witness_is_rejected(bpg, reg, edge, entry):
    """the forged row replaces row 9 of the device's edge trace: the device checker names it, the prover proves what it
    is given, the verifier rejects at zeta"""
    _, t = edge
    bad = t.clone()
    bad[:, 9] = to_dev(np.array(model.forged(entry), dtype=np.uint64))
    got = bpg.ops.check_air_trace(reg, bad, max_viol=512)
    assert got.rows == [9] and {am.FAMILIES[v.family][0] for v in got.violations} == entry[3]
    cfg = cfg_of(reg, 5)
    assert cases.verify(reg, cfg, bpg.ops.stark_prove_trace(reg, cfg, bad)) == -5
    assert b"constraint check at zeta" in bpg.lib().bp_last_error()


def test_the_ports_running_products_are_the_builders(bpg, reg, edge):
    ops, t = edge
    assert 0 < sum(1 for op in ops if op[0] in (1, 2) and op[4]) < 32
    rng = np.random.default_rng(0xA07C)
    ctl = [int(v) for v in rng.integers(2, model.P, size=4, dtype=np.uint64)]
    got = to_host(bpg.ops.air_port_products(reg, t, ctl))
    want = am.program().port_running_columns(model.trace_of(ops), ctl)
    assert got.shape == (2, 32) and [[int(v) for v in col] for col in got] == want
    assert int(got[0, 0]) not in (0, 1) and int(got[0, 0]) != int(got[1, 0])


# ---------------------------------------------------------------------------------------------- table sets
WIDTH, LOOKER_COLS = 66, 72     # the looking table: pc.flag_program's flag column and the port's 66-element tuple


def tuple_of(op, a, b, m, res):
    return [int(op == model.ADDMOD), int(op == model.MULMOD)] + model.limbs(a) + model.limbs(b) + model.limbs(m) + model.limbs(res)


def honest_claim(op, a, b, m, _=None):
    u = a + b if op == model.ADDMOD else a * b
    return (op, a, b, m, u % m if m else 0)


def modular_set(bpg, reg, ops, claims, seed):
    """(statement, [looking trace (numpy), modular trace (device)], looking rows): a 2^5-row modular table of `ops` and a
    2^4-row table that sends `claims` = [(op, a, b, m, res), ...]"""
    looker = bpg.ops.air_register(pc.flag_program(width=WIDTH, n_cols=LOOKER_COLS).assemble())
    rng = np.random.default_rng(seed)
    rows = pc.rows_of(4, rng, len(claims))
    a = pc.flagged(4, rows, [tuple_of(*c) for c in claims], rng, width=WIDTH, n_cols=LOOKER_COLS)
    tables = [{"air_id": looker, "cfg": cfg_of(looker, 4)}, {"air_id": reg, "cfg": cfg_of(reg, 5)}]
    return tables, [a, device_trace(bpg, ops)], rows


def with_traces(tables, traces):
    return [dict(tables[0], trace=to_dev(traces[0])), dict(tables[1], trace=traces[1])]


def refused_by_the_pre_flight_the_prover_and_the_verifier(bpg, tables, traces, looking_row, looked_row):
    from proof_protocol_decoder_amd._lib import BpgError
    full = with_traces(tables, traces)
    got = bpg.ops.check_table_set(full, LINK)
    assert not got.ok and all(t.ok for t in got.tables) and "link 0 does not balance" in got.message, got.message
    assert "looking row %d (port 0 of table 0)" % looking_row in got.message
    lk, = got.links
    assert not lk.holds and (lk.first_looking_end, lk.first_looking_row, lk.first_looked_row) == (0, looking_row, looked_row), lk
    with pytest.raises(BpgError) as e:
        bpg.ops.stark_prove_table_set(full, LINK)
    assert e.value.code == -5 and "link 0 does not hold" in e.value.message
    container = bpg.ops.stark_prove_table_set(full, LINK, skip_link_check=True)
    with pytest.raises(BpgError) as e:
        bpg.ops.stark_verify_table_set(tables, LINK, container)
    assert e.value.code == -5 and "link 0 does not hold" in e.value.message


# rows of the edge list: both carry extremes, a product over m = 0, (2^256 - 1)^2 mod 1, a 257-bit q, r = m - 1 under
# either operation, a sum over m = 2^256 - 1
ASKED = [0, 1, 3, 5, 10, 12, 13, 8]


def test_a_callers_table_looks_modular_operations_up(bpg, reg):
    edge_ops = model.edge_ops()
    assert {edge_ops[i][0] for i in ASKED} == {model.ADDMOD, model.MULMOD}
    ops = [(op, a, b, m, int(i in ASKED)) for i, (op, a, b, m, _) in enumerate(edge_ops)]
    claims = [honest_claim(*edge_ops[i]) for i in reversed(ASKED)]                # ... in another order
    tables, traces, _ = modular_set(bpg, reg, ops, claims, 0xA075)
    full = with_traces(tables, traces)
    got = bpg.ops.check_table_set(full, LINK)
    assert got.ok and got.links[0].holds and (got.links[0].n_looking, got.links[0].n_looked) == (8, 8), got
    container = bpg.ops.stark_prove_table_set(full, LINK)
    bpg.ops.stark_verify_table_set(tables, LINK, container)


A_, B_ = (1 << 256) - 3, 10          # a + b = 2^256 + 7: (a + b) mod 9 = 5, but ((a + b) mod 2^256) mod 9 = 7
assert (A_ + B_) % 9 == 5 and ((A_ + B_) % (1 << 256)) % 9 == 7


def one_addmod(bpg, reg, exposed, res):
    """the modular table's row 21 (a padding row of the edge list) replaced by ADDMOD(2^256 - 3, 10, 9), the only claim
    of the looking table"""
    ops = [(op, a, b, m, 0) for op, a, b, m, _ in model.edge_ops()]
    assert ops[21][0] not in (model.ADDMOD, model.MULMOD)
    ops[21] = (model.ADDMOD, A_, B_, 9, exposed)
    tables, traces, rows = modular_set(bpg, reg, ops, [(model.ADDMOD, A_, B_, 9, res)], 0xA076)
    return tables, traces, rows[0]


def test_the_sum_is_reduced_over_the_integers(bpg, reg):
    tables, traces, _ = one_addmod(bpg, reg, 1, 5)
    full = with_traces(tables, traces)
    assert bpg.ops.check_table_set(full, LINK).ok
    bpg.ops.stark_verify_table_set(tables, LINK, bpg.ops.stark_prove_table_set(full, LINK))


def test_a_claim_of_the_wrapped_sums_answer_is_refused(bpg, reg):
    tables, traces, row = one_addmod(bpg, reg, 1, 7)
    refused_by_the_pre_flight_the_prover_and_the_verifier(bpg, tables, traces, row, 21)


def test_an_operation_that_is_not_exposed_cannot_be_looked_up(bpg, reg):
    tables, traces, row = one_addmod(bpg, reg, 0, 5)
    refused_by_the_pre_flight_the_prover_and_the_verifier(bpg, tables, traces, row, -1)


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(bpg):
    import torch
    from proof_protocol_decoder_amd._lib import BpgError
    good = to_dev(am.pack_inputs(model.edge_ops()))
    with pytest.raises(BpgError) as e:
        bpg.ops.arithmetic_mod_trace(5, None)
    assert e.value.code == -2 and "null inputs" in e.value.message
    with pytest.raises(ValueError, match=r"\[32, 13\]"):
        bpg.ops.arithmetic_mod_trace(5, good[:31])
    with pytest.raises(ValueError, match=r"\[16, 13\]"):
        bpg.ops.arithmetic_mod_trace(4, good)
    with pytest.raises(ValueError, match=r"\[32, 13\]"):
        bpg.ops.arithmetic_mod_trace(5, torch.zeros((32, 9), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="int64"):
        bpg.ops.arithmetic_mod_trace(5, good.to(torch.int32))
    with pytest.raises(ValueError, match="device tensors"):
        bpg.ops.arithmetic_mod_trace(5, good.cpu())
    # heights outside 4 .. 26 are refused before anything is launched, so the pointers are never read
    out = torch.zeros(8, dtype=torch.int64, device="cuda")
    for log_n in (3, 27):
        assert bpg.lib().bp_arithmetic_mod_trace(good.data_ptr(), log_n, out.data_ptr(), None) == -2
        assert b"log_n out of range" in bpg.lib().bp_last_error()
    assert bpg.lib().bp_arithmetic_mod_trace(good.data_ptr(), 5, None, None) == -2
    torch.cuda.synchronize()
    assert int(out.sum()) == 0
