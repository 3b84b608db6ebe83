"""The division table on the GPU: the witness kernel (csrc/arithmetic_div.hip) against the independent row model of
tests/arithmetic_div_model.py word for word, then the shipped program through the run-time stack -- the device checker,
the prover and the verifier, the port's running products, and table sets in which a caller's table looks divisions up.
Everything is exact.  CPU side: tests/test_arithmetic_div.py."""
import numpy as np
import pytest

import air_program_cases as cases
import air_program_port_cases as pc
import arithmetic_div_model as model
from air_program_port_cases import LINK, cfg_of
from proof_protocol_decoder_amd import arithmetic_div as ad
from util import to_dev, to_host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def reg(bpg):
    return ad.register()


def device_trace(bpg, ops):
    log_n = len(ops).bit_length() - 1
    return bpg.ops.arithmetic_div_trace(log_n, to_dev(ad.pack_inputs(ops)))


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
    ops = {"edges-2^5": model.edge_ops, "edges-2^7": model.edge_ops_full, "random-2^9": lambda: model.random_ops(512, 0x9D1F)}[which]()
    t = device_trace(bpg, ops)
    assert_equal_word_for_word(to_host(t), model.trace_of(ops))
    got = bpg.ops.check_air_trace(reg, t)
    assert got.ok and got.n_violations == 0, got


def test_the_kernel_writes_every_cell_and_ignores_what_it_should(bpg):
    """a trace buffer full of ones before the call; bits 9 .. 63 of word 0 and a padding row's operands change nothing"""
    import torch
    ops = model.edge_ops()
    words = ad.pack_inputs(ops)
    want = model.trace_of(ops)
    words[:, 0] |= np.uint64(0xABCDEF << 9)
    out = torch.full((ad.N_COLS, 32), -1, dtype=torch.int64, device="cuda")
    d_words = to_dev(words)
    assert bpg.lib().bp_arithmetic_div_trace(d_words.data_ptr(), 5, out.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    assert_equal_word_for_word(to_host(out), want)


def test_the_edge_trace_proves_and_verifies(bpg, reg, edge):
    _, t = edge
    cfg = cases.cfg_for(reg, 5)
    assert (cfg.n_cols, cfg.rate_bits, cfg.deg_pow) == (1650, 1, 1)
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
    assert got.rows == [9] and {ad.FAMILIES[v.family][0] for v in got.violations} == entry[3]
    cfg = cfg_of(reg, 5)
    assert cases.verify(reg, cfg, bpg.ops.stark_prove_trace(reg, cfg, bad)) == -5
    assert b"constraint check at zeta" in bpg.lib().bp_last_error()


def test_the_ports_running_products_are_the_builders(bpg, reg, edge):
    ops, t = edge
    assert 0 < sum(1 for op in ops if op[0] in (1, 2) and op[3]) < 32
    rng = np.random.default_rng(0xD17C)
    ctl = [int(v) for v in rng.integers(2, model.P, size=4, dtype=np.uint64)]
    got = to_host(bpg.ops.air_port_products(reg, t, ctl))
    want = ad.program().port_running_columns(model.trace_of(ops), ctl)
    assert got.shape == (2, 32) and [[int(v) for v in col] for col in got] == want
    assert int(got[0, 0]) not in (0, 1) and int(got[0, 0]) != int(got[1, 0])


# ---------------------------------------------------------------------------------------------- table sets
WIDTH = 50     # the looking table: pc.flag_program's flag column and the port's 50-element tuple


def tuple_of(op, x, y, res):
    return [int(op == model.DIV), int(op == model.MOD)] + model.limbs(x) + model.limbs(y) + model.limbs(res)


def division_set(bpg, reg, asked, claims):
    """(statement, [looking trace (numpy), division trace (device)]): a 2^5-row division table that exposes the rows
    `asked` of the edge list and nothing else, and a 2^4-row table that sends `claims` = [(op, x, y, res), ...]"""
    looker = bpg.ops.air_register(pc.flag_program(width=WIDTH, n_cols=56).assemble())
    ops = [(op, x, y, int(i in asked)) for i, (op, x, y, _) in enumerate(model.edge_ops())]
    rng = np.random.default_rng(0xD175)
    rows = pc.rows_of(4, rng, len(claims))
    a = pc.flagged(4, rows, [tuple_of(*c) for c in claims], rng, width=WIDTH, n_cols=56)
    tables = [{"air_id": looker, "cfg": cfg_of(looker, 4)}, {"air_id": reg, "cfg": cfg_of(reg, 5)}]
    return tables, [a, device_trace(bpg, ops)], rows


def honest_claim(op, x, y, _=None):
    q, r = divmod(x, y) if y else (0, x)
    return (op, x, y, 0 if y == 0 else q if op == model.DIV else r)


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


ASKED = [1, 7, 8, 12, 17, 2]   # rows of the edge list: x / 0, MAX % MAX, MAX / 2, a top-limb y, the largest carry, y = 1


def test_a_callers_table_looks_divisions_up(bpg, reg):
    edge_ops = model.edge_ops()
    claims = [honest_claim(*edge_ops[i]) for i in reversed(ASKED)]                # ... in another order
    tables, traces, _ = division_set(bpg, reg, ASKED, claims)
    full = with_traces(tables, traces)
    got = bpg.ops.check_table_set(full, LINK)
    assert got.ok and got.links[0].holds and (got.links[0].n_looking, got.links[0].n_looked) == (6, 6), got
    container = bpg.ops.stark_prove_table_set(full, LINK)
    bpg.ops.stark_verify_table_set(tables, LINK, container)


def seven_by_two(bpg, reg, exposed, res):
    """the division table's row 20 (a padding row of the edge list) replaced by 7 / 2, the only claim of the looking table"""
    looker = bpg.ops.air_register(pc.flag_program(width=WIDTH, n_cols=56).assemble())
    ops = [(op, x, y, 0) for op, x, y, _ in model.edge_ops()]
    ops[20] = (model.DIV, 7, 2, exposed)
    rng = np.random.default_rng(0xD176)
    rows = pc.rows_of(4, rng, 1)
    a = pc.flagged(4, rows, [tuple_of(model.DIV, 7, 2, res)], rng, width=WIDTH, n_cols=56)
    tables = [{"air_id": looker, "cfg": cfg_of(looker, 4)}, {"air_id": reg, "cfg": cfg_of(reg, 5)}]
    return tables, [a, device_trace(bpg, ops)], rows[0]


def test_seven_by_two_is_three(bpg, reg):
    tables, traces, _ = seven_by_two(bpg, reg, 1, 3)
    full = with_traces(tables, traces)
    assert bpg.ops.check_table_set(full, LINK).ok
    bpg.ops.stark_verify_table_set(tables, LINK, bpg.ops.stark_prove_table_set(full, LINK))


def test_a_claim_that_seven_by_two_is_four_is_refused(bpg, reg):
    tables, traces, row = seven_by_two(bpg, reg, 1, 4)
    refused_by_the_pre_flight_the_prover_and_the_verifier(bpg, tables, traces, row, 20)


def test_a_division_that_is_not_exposed_cannot_be_looked_up(bpg, reg):
    tables, traces, row = seven_by_two(bpg, reg, 0, 3)
    refused_by_the_pre_flight_the_prover_and_the_verifier(bpg, tables, traces, row, -1)


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(bpg):
    import torch
    from proof_protocol_decoder_amd._lib import BpgError
    good = to_dev(ad.pack_inputs(model.edge_ops()))
    with pytest.raises(BpgError) as e:
        bpg.ops.arithmetic_div_trace(5, None)
    assert e.value.code == -2 and "null inputs" in e.value.message
    with pytest.raises(ValueError, match=r"\[32, 9\]"):
        bpg.ops.arithmetic_div_trace(5, good[:31])
    with pytest.raises(ValueError, match=r"\[16, 9\]"):
        bpg.ops.arithmetic_div_trace(4, good)
    with pytest.raises(ValueError, match=r"\[32, 9\]"):
        bpg.ops.arithmetic_div_trace(5, torch.zeros((32, 8), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="int64"):
        bpg.ops.arithmetic_div_trace(5, good.to(torch.int32))
    with pytest.raises(ValueError, match="device tensors"):
        bpg.ops.arithmetic_div_trace(5, good.cpu())
    # the heights bp_arithmetic_mul_trace takes: refused before anything is launched, so the pointers are never read
    out = torch.zeros(8, dtype=torch.int64, device="cuda")
    for log_n in (3, 27):
        assert bpg.lib().bp_arithmetic_div_trace(good.data_ptr(), log_n, out.data_ptr(), None) == -2
        assert b"log_n out of range" in bpg.lib().bp_last_error()
    assert bpg.lib().bp_arithmetic_div_trace(good.data_ptr(), 5, None, None) == -2
    torch.cuda.synchronize()
    assert int(out.sum()) == 0
