"""The shift table on the CPU: the shipped program (proof_protocol_decoder_amd/arithmetic_shift.py) against the
independent row model of tests/arithmetic_shift_model.py -- the column maps, Builder.evaluate over Python integers, the
library's host checker -- and a catalogue of wrong witnesses, each named at its row and family.  The fixtures and the
tests it has in common with the other shipped tables are word_tables.cpu_tests over this table's record; its own follow.
Nothing here needs a GPU; the device side is tests/test_gpu_arithmetic_shift.py."""
import pytest

import arithmetic_shift_model as model
from proof_protocol_decoder_amd import arithmetic_shift as sh
from word_tables import SHIFT, cpu_tests

globals().update(cpu_tests(SHIFT))


def test_every_unit_cut_states_the_same_constraints():
    row = model.cells(model.honest(model.SAR, 0x47, model.G1, 1))
    bad = model.forged(model.CATALOGUE[7])
    want = sh.program().evaluate(bad, bad)
    assert any(want)
    for cut in sh.CUTS:
        p = sh.program(cut)
        # a register is 2 KiB of a workgroup's LDS: the shipped cut needs no more than the division table's 8
        assert len(p.units) == 1 + 16 // cut and int(p.assemble()[7]) <= (8 if cut == sh.LIMBS_PER_UNIT else 16)
        assert not any(p.evaluate(row, row)) and p.evaluate(bad, bad) == want
    with pytest.raises(ValueError):
        sh.program(3)


def test_the_edge_list_covers_what_the_statement_singles_out():
    ops = model.edge_ops()
    assert len(ops) == 32 and len(model.edge_ops_full()) == 128
    assert all(ops[i][0] not in model.LIVE for i in model.PADDING_ROWS) and 9 in model.PADDING_ROWS
    for collection in (ops, model.edge_ops_full()):
        counts, values = {o[1] for o in collection if o[0] in model.LIVE}, {o[2] for o in collection if o[0] in model.LIVE}
        assert {0, 1, 15, 16, 17, 255, 256, 257, 0x300, (1 << 16) + 5, 1 << 255, model.MAX} <= counts
        assert {0, 1, 1 << 255, (1 << 255) - 1, model.MAX} <= values
        sar_negative = {o[1] for o in collection if o[0] == model.SAR and o[2] >> 255}
        assert 255 in sar_negative and any(s >= 256 for s in sar_negative)
    below = sum(1 for o in model.random_ops(1000, 1) if o[1] < 256)
    assert 450 < below < 650                                   # half the draws, and the short words of the other half


def test_the_model_rows_state_the_evm_operations():
    """the model's limb-wise witness against the statement itself, and the masked count giving another answer"""
    for op, s, x, e in model.edge_ops_full() + model.random_ops(400, 0x5F72):
        w = model.honest(op, s, x, e)
        if op not in model.LIVE:
            assert model.word(w["resl"]) == model.word(w["sl"]) == model.word(w["xl"]) == 0 and w["g"] == 0
            assert (w["z"], w["l"][0], w["e"][15], w["W"]) == (1, 1, 1, 0) and not any(w["y"] + w["lo"] + w["hi"])
            continue
        signed = x - (x >> 255 << 256)
        want = {model.SHL: (x << min(s, 256)) & model.M256, model.SHR: x >> min(s, 256), model.SAR: (signed >> min(s, 256)) & model.M256}[op]
        assert model.word(w["resl"]) == want == model.statement(op, s, x)
    assert model.statement(model.SHL, 256, 5) == 0 != model.statement(model.SHL, 0, 5)


def test_the_largest_values_are_below_the_field(program):
    """AIRS.md: x_k W < 2^32, T < 2^20, |sum d e_d| <= 15 -- the edge rows reach the first two"""
    w = model.honest(model.SHR, model.MAX, model.MAX, 1)
    assert w["W"] == 2 and sum(w["sl"][1:]) + 0xFF == 15 * 0xFFFF + 0xFF < 1 << 20
    w = model.honest(model.SAR, 0, model.MAX, 1)
    assert w["W"] == 1 << 16 and max(xk * w["W"] for xk in w["xl"]) == 0xFFFF0000 < model.P


def test_the_catalogue_breaks_every_family():
    assert set().union(*(e[3] for e in model.CATALOGUE)) == {name for name, _ in model.FAMILIES}
