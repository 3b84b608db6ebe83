"""The signed table on the CPU: the shipped program (proof_protocol_decoder_amd/arithmetic_sdiv.py) against the
independent row model of tests/arithmetic_sdiv_model.py -- the column maps, Builder.evaluate over Python integers, the
library's host checker -- and a catalogue of wrong witnesses, each named at its row and family.  The fixtures and the
tests it has in common with the other shipped tables are word_tables.cpu_tests over this table's record; its own follow.
Nothing here needs a GPU; the device side is tests/test_gpu_arithmetic_sdiv.py."""
import math
from fractions import Fraction

import pytest

import arithmetic_sdiv_model as model
from proof_protocol_decoder_amd import arithmetic_div, arithmetic_sdiv as sd
from word_tables import SIGNED, cpu_tests, signed

globals().update(cpu_tests(SIGNED))


def test_a_table_that_looks_divisions_up_fits_this_one():
    """the division table's port has the same width -- the same flags-and-three-words tuple -- and its input words are
    this table's"""
    assert len(arithmetic_div.TUPLE_COLS) == len(sd.TUPLE_COLS) == SIGNED.width
    ops = model.edge_ops()
    assert (sd.pack_inputs(ops) == arithmetic_div.pack_inputs(ops)).all()


def test_every_unit_cut_states_the_same_constraints():
    row = model.cells(model.honest(model.SMOD, model.to_word(-model.EXTREME), model.HALF, 1))
    bad = model.forged(model.CATALOGUE[0])
    want = sd.program().evaluate(bad, bad)
    assert any(want)
    assert sd.CUTS == (1, 2) and sd.LIMBS_PER_UNIT in sd.CUTS
    for cut in sd.CUTS:
        p = sd.program(cut)
        # a register is 2 KiB of a workgroup's LDS: no cut needs more than 16
        assert len(p.units) == 1 + 16 // cut and int(p.assemble()[7]) <= 16
        assert not any(p.evaluate(row, row)) and p.evaluate(bad, bad) == want
    with pytest.raises(ValueError):
        sd.program(4)


def test_the_edge_list_covers_what_the_statement_singles_out():
    ops = model.edge_ops()
    assert len(ops) == 32 and len(model.edge_ops_full()) == 128
    assert all(ops[i][0] not in model.LIVE for i in model.PADDING_ROWS) and 9 in model.PADDING_ROWS
    n_ = model.to_word
    operands = {0, 1, 2, 7, n_(-1), n_(-2), n_(-7), (1 << 255) - 1, 1 << 255, n_(1 - (1 << 255)), model.HALF, n_(-model.HALF),
                1 << 128, n_(-(1 << 128))}
    rows = {(1 << 255, n_(-1)), (1 << 255, 1), (n_(-7), 2), (7, n_(-2)), (n_(-7), n_(-2)), (n_(-8), 2), (n_(-1), 1 << 255),
            (model.EXTREME, model.HALF), (n_(-model.EXTREME), model.HALF)}
    for collection in (ops, model.edge_ops_full()):
        live = [o for o in collection if o[0] in model.LIVE]
        assert operands <= {o[1] for o in live} and operands <= {o[2] for o in live}      # every edge operand in both positions
        assert rows <= {o[1:3] for o in live}
        assert {o[1] >> 255 for o in live if o[2] == 0} == {0, 1}                          # (x, 0) under both signs of x
        assert {o[0] for o in live} == set(model.LIVE)
    full = model.edge_ops_full()
    assert all((op, x, y, e) in full for x, y in model.EDGE_PAIRS for op in model.LIVE for e in (0, 1))
    negative = sum(1 for o in model.random_ops(1000, 1) if o[1] >> 255)
    assert 400 < negative < 600


def test_the_model_rows_state_the_evm_operations():
    """the model's witness, which divides magnitudes, against the statement written a second way: Python's signed
    integers and an explicit truncation toward zero (never //, which floors)"""
    for op, x, y, e in model.edge_ops_full() + model.random_ops(400, 0x5D12):
        w = model.honest(op, x, y, e)
        res = model.word(w["resl"])
        if op not in model.LIVE:
            assert res == model.word(w["xl"]) == model.word(w["yl"]) == 0 and (w["g"], w["z"], w["neg"]) == (0, 1, 0)
            continue
        sx, sy = signed(x), signed(y)
        if sy == 0:
            assert res == 0 and w["z"] == 1
            continue
        quotient = math.trunc(Fraction(sx, sy))
        remainder = sx - sy * quotient
        assert abs(remainder) < abs(sy) and (remainder == 0 or (remainder < 0) == (sx < 0))   # the sign of the dividend
        assert res == (quotient if op == model.SDIV else remainder) % (1 << 256) == model.statement(op, x, y)
        assert model.word(w["ql"]) == abs(quotient) and w["rb"] == abs(remainder)
    n_ = model.to_word
    # the two classic mistakes, and the quotient that has no positive word
    assert signed(model.statement(model.SDIV, n_(-7), 2)) == -3 != -7 // 2
    assert signed(model.statement(model.SMOD, n_(-7), 2)) == -1 != -7 % 2
    assert signed(model.statement(model.SMOD, 7, n_(-2))) == 1 != 7 % -2
    assert model.statement(model.SDIV, 1 << 255, n_(-1)) == 1 << 255 and model.statement(model.SMOD, 1 << 255, n_(-1)) == 0
    assert model.statement(model.SDIV, n_(-8), 2) == n_(-4) and model.statement(model.SMOD, n_(-8), 2) == 0
    assert model.statement(model.SDIV, 5, 0) == model.statement(model.SMOD, n_(-5), 0) == 0


def test_the_largest_values_are_below_the_field():
    """AIRS.md: the largest carry a search found, 0x77FF8 out of column 7 under either sign of x, needs all 19 bits; a
    product column stays below 2^37, a chain limb below 2^18"""
    for x in (model.EXTREME, model.to_word(-model.EXTREME)):
        w = model.honest(model.SDIV, x, model.HALF, 1)
        assert max(w["carry"]) == w["carry"][7] == model.LARGEST_CARRY and model.LARGEST_CARRY >> 18 == 1
        assert w["rb"] == model.HALF - 1 and model.word(w["ql"]) == (1 << 127) - 1
    assert max(max(model.honest(*op)["carry"]) for op in model.edge_ops_full() + model.random_ops(400, 0x5D13)) == model.LARGEST_CARRY
    assert 16 * 0xFFFF * 0xFFFF + 0xFFFF + (1 << 19) < 1 << 37 < model.P and 2 * 0xFFFF + 1 < 1 << 18
    w = model.honest(model.SDIV, 1 << 255, model.to_word(-1), 1)               # the magnitude 2^255, which no positive word holds
    assert w["axb"] == 1 << 255 == w["qb"] == w["resb"] and w["neg"] == 0 and w["cx"][15] == 1


def test_the_catalogue_breaks_every_family():
    assert set().union(*(e[3] for e in model.CATALOGUE)) == {name for name, _ in model.FAMILIES}
    assert len({e[0] for e in model.CATALOGUE}) == len(model.CATALOGUE)
