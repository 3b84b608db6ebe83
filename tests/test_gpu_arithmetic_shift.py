"""The shift table on the GPU: the witness kernel (csrc/arithmetic_shift.hip) against the independent row model of
tests/arithmetic_shift_model.py word for word, then the shipped program through the run-time stack -- the device checker,
the prover and the verifier, the port's running products, and table sets in which a caller's table looks shifts up.
Everything is exact.  The bodies restate word_tables.gpu_tests for a table of three operations (a 51-element tuple with
three flags); what holds unchanged is imported from there.  The stories of the masked count are its own.  CPU side:
tests/test_arithmetic_shift.py."""
from types import SimpleNamespace

import numpy as np
import pytest

import air_program_cases as cases
import air_program_port_cases as pc
import arithmetic_shift_model as model
from air_program_port_cases import LINK, cfg_of
from proof_protocol_decoder_amd import arithmetic_shift as sh
from util import to_dev, to_host
from word_tables import (assert_equal_word_for_word, device_trace, proves_and_verifies,
                         refused_by_the_pre_flight_the_prover_and_the_verifier, with_traces)

pytestmark = pytest.mark.gpu

SHIFT = SimpleNamespace(name="shift", module=sh, model=model, trace_op="arithmetic_shift_trace")
N_COLS, WIDTH, LOOKER_COLS = 1143, 51, 57
# rows of the edge list a caller asks for: SHL by 0 and by 16, SHR by 1 and past 256, SAR by 15 and by 0x300, SHL by 2^16 + 5
ASKED = [0, 3, 1, 7, 2, 8, 10]


@pytest.fixture(scope="module")
def reg(bpg):
    return sh.register()


@pytest.fixture(scope="module")
def edge(bpg):
    """(operations, device trace) of the 2^5-row edge list"""
    ops = model.edge_ops()
    return ops, device_trace(bpg, SHIFT, ops)


# 2^5: fewer rows than a workgroup; 2^7: every edge under all three flags, exposed and not; 2^9: two workgroups
@pytest.mark.parametrize("which", ["edges-2^5", "edges-2^7", "random-2^9"])
def test_the_device_witness_is_the_model_and_the_checker_is_clean(bpg, reg, which):
    ops = {"edges-2^5": model.edge_ops, "edges-2^7": model.edge_ops_full, "random-2^9": lambda: model.random_ops(512, 0x5F1F)}[which]()
    t = device_trace(bpg, SHIFT, ops)
    assert_equal_word_for_word(to_host(t), model.trace_of(ops))
    got = bpg.ops.check_air_trace(reg, t)
    assert got.ok and got.n_violations == 0, got


def test_the_kernel_writes_every_cell_and_ignores_what_it_should(bpg):
    """a trace buffer full of ones before the call; bits 9 .. 63 of word 0 and a padding row's operands change nothing"""
    import torch
    ops = model.edge_ops()
    words = sh.pack_inputs(ops)
    want = model.trace_of(ops)
    words[:, 0] |= np.uint64(0xABCDEF << 9)
    assert any(int(words[i, 1:].any()) for i, op in enumerate(ops) if op[0] not in model.LIVE)   # padding rows carry junk
    out = torch.full((N_COLS, 32), -1, dtype=torch.int64, device="cuda")
    d_words = to_dev(words)
    assert bpg.lib().bp_arithmetic_shift_trace(d_words.data_ptr(), 5, out.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    assert_equal_word_for_word(to_host(out), want)


def test_the_edge_trace_proves_and_verifies(bpg, reg, edge):
    _, t = edge
    cfg = cases.cfg_for(reg, 5)
    assert (cfg.n_cols, cfg.rate_bits, cfg.deg_pow) == (N_COLS, 1, 1)
    proof = bpg.ops.stark_prove_trace(reg, cfg, t)
    assert int(proof[4]) == 2 and int(proof[14]) == reg                         # two auxiliary columns: the port's products
    bpg.ops.stark_verify_air(reg, cfg, proof)
    assert cases.verify(7, cases.cfg_for(7, 5), proof) == -5                    # ... under its own id only


@pytest.mark.parametrize("entry", model.CATALOGUE, ids=[e[0] for e in model.CATALOGUE])
def test_the_proof_of_a_wrong_witness_is_rejected(bpg, reg, edge, entry):
    """the forged row replaces row 9 of the device's edge trace: the device checker names it, the prover proves what it is
    given, the verifier rejects at zeta"""
    _, t = edge
    bad = t.clone()
    bad[:, 9] = to_dev(np.array(model.forged(entry), dtype=np.uint64))
    got = bpg.ops.check_air_trace(reg, bad, max_viol=512)
    assert got.rows == [9] and {sh.FAMILIES[v.family][0] for v in got.violations} == entry[3]
    cfg = cfg_of(reg, 5)
    assert cases.verify(reg, cfg, bpg.ops.stark_prove_trace(reg, cfg, bad)) == -5
    assert b"constraint check at zeta" in bpg.lib().bp_last_error()


def test_the_ports_running_products_are_the_builders(bpg, reg, edge):
    ops, t = edge
    assert 0 < sum(1 for op in ops if op[0] in model.LIVE and op[3]) < 32
    rng = np.random.default_rng(0x5F7C)
    ctl = [int(v) for v in rng.integers(2, model.P, size=4, dtype=np.uint64)]
    got = to_host(bpg.ops.air_port_products(reg, t, ctl))
    want = sh.program().port_running_columns(model.trace_of(ops), ctl)
    assert got.shape == (2, 32) and [[int(v) for v in col] for col in got] == want
    assert int(got[0, 0]) not in (0, 1) and int(got[0, 0]) != int(got[1, 0])


# ---------------------------------------------------------------------------------------------- table sets
def tuple_of(op, s, x, res):
    """the port's tuple: the three flags, then the limbs of s, of x and of the result"""
    return [int(op == o) for o in model.LIVE] + model.limbs(s) + model.limbs(x) + model.limbs(res)


def table_set(bpg, reg, ops, claims, seed):
    """(statement, [looking trace (numpy), the table's trace (device)], looking rows): a 2^5-row table of `ops` and a
    2^4-row table -- pc.flag_program's flag column and the port's tuple -- that sends `claims` = [(op, s, x, res), ...]"""
    looker = bpg.ops.air_register(pc.flag_program(width=WIDTH, n_cols=LOOKER_COLS).assemble())
    rng = np.random.default_rng(seed)
    rows = pc.rows_of(4, rng, len(claims))
    a = pc.flagged(4, rows, [tuple_of(*c) for c in claims], rng, width=WIDTH, n_cols=LOOKER_COLS)
    tables = [{"air_id": looker, "cfg": pc.cfg_of(looker, 4)}, {"air_id": reg, "cfg": pc.cfg_of(reg, 5)}]
    return tables, [a, device_trace(bpg, SHIFT, ops)], rows


def one_claim(bpg, reg, operation, exposed, res, seed):
    """row 9 of the edge list (a padding row, nothing else exposed) replaced by `operation` = (op, s, x), the only claim
    of the looking table, which claims `res` for it; returns (statement, traces, looking row)"""
    ops = [o[:-1] + (0,) for o in model.edge_ops()]
    assert ops[9][0] not in model.LIVE
    ops[9] = operation + (exposed,)
    tables, traces, rows = table_set(bpg, reg, ops, [operation + (res,)], seed)
    return tables, traces, rows[0]


def test_a_callers_table_looks_shifts_up(bpg, reg):
    """the table exposes the rows ASKED of the edge list and nothing else; the caller claims them in another order"""
    edge_ops = model.edge_ops()
    assert {edge_ops[i][0] for i in ASKED} == set(model.LIVE)
    ops = [o[:-1] + (int(i in ASKED),) for i, o in enumerate(edge_ops)]
    claims = [edge_ops[i][:3] + (model.statement(*edge_ops[i][:3]),) for i in reversed(ASKED)]
    tables, traces, _ = table_set(bpg, reg, ops, claims, 0x5F75)
    full = with_traces(tables, traces)
    got = bpg.ops.check_table_set(full, LINK)
    n = len(ASKED)
    assert got.ok and got.links[0].holds and (got.links[0].n_looking, got.links[0].n_looked) == (n, n), got
    container = bpg.ops.stark_prove_table_set(full, LINK)
    bpg.ops.stark_verify_table_set(tables, LINK, container)


X_ = model.G2                                  # SHL(256, x) = 0, and x itself if only the count's low byte were read
NEG = model.G1                                 # a negative word: SAR(2^16 + 5, x) is all ones, SAR(5, x) is not
assert model.statement(model.SHL, 256, X_) == 0 and model.statement(model.SHL, 256 & 0xFF, X_) == X_
assert model.statement(model.SAR, model.LIMB_ONE, NEG) == model.MAX != model.statement(model.SAR, 5, NEG)


def test_a_shift_by_256_is_zero(bpg, reg):
    tables, traces, _ = one_claim(bpg, reg, (model.SHL, 256, X_), 1, 0, 0x5F76)
    proves_and_verifies(bpg, tables, traces)


def test_a_claim_of_the_masked_counts_answer_is_refused(bpg, reg):
    tables, traces, row = one_claim(bpg, reg, (model.SHL, 256, X_), 1, X_, 0x5F76)
    refused_by_the_pre_flight_the_prover_and_the_verifier(bpg, tables, traces, row, 9)


def test_sar_past_the_word_is_the_sign(bpg, reg):
    tables, traces, _ = one_claim(bpg, reg, (model.SAR, model.LIMB_ONE, NEG), 1, model.MAX, 0x5F77)
    proves_and_verifies(bpg, tables, traces)


def test_a_claim_of_sar_by_the_masked_count_is_refused(bpg, reg):
    tables, traces, row = one_claim(bpg, reg, (model.SAR, model.LIMB_ONE, NEG), 1, model.statement(model.SAR, 5, NEG), 0x5F77)
    refused_by_the_pre_flight_the_prover_and_the_verifier(bpg, tables, traces, row, 9)


def test_an_operation_that_is_not_exposed_cannot_be_looked_up(bpg, reg):
    tables, traces, row = one_claim(bpg, reg, (model.SHL, 256, X_), 0, 0, 0x5F76)
    refused_by_the_pre_flight_the_prover_and_the_verifier(bpg, tables, traces, row, -1)


def test_refusals(bpg):
    import torch
    from proof_protocol_decoder_amd._lib import BpgError
    trace = bpg.ops.arithmetic_shift_trace
    good = to_dev(sh.pack_inputs(model.edge_ops()))
    with pytest.raises(BpgError) as e:
        trace(5, None)
    assert e.value.code == -2 and "null inputs" in e.value.message
    with pytest.raises(ValueError, match=r"\[32, 9\]"):
        trace(5, good[:31])
    with pytest.raises(ValueError, match=r"\[16, 9\]"):
        trace(4, good)
    with pytest.raises(ValueError, match=r"\[32, 9\]"):
        trace(5, torch.zeros((32, 8), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="int64"):
        trace(5, good.to(torch.int32))
    with pytest.raises(ValueError, match="device tensors"):
        trace(5, good.cpu())
    # heights outside 4 .. 26 are refused before anything is launched, so the pointers are never read
    entry = bpg.lib().bp_arithmetic_shift_trace
    out = torch.zeros(8, dtype=torch.int64, device="cuda")
    for log_n in (3, 27):
        assert entry(good.data_ptr(), log_n, out.data_ptr(), None) == -2
        assert b"log_n out of range" in bpg.lib().bp_last_error()
    assert entry(good.data_ptr(), 5, None, None) == -2
    torch.cuda.synchronize()
    assert int(out.sum()) == 0
