"""The modular table on the CPU: the shipped program (proof_protocol_decoder_amd/arithmetic_mod.py) against the
independent row model of tests/arithmetic_mod_model.py -- the column maps, Builder.evaluate over Python integers, the
library's host checker -- and a catalogue of wrong witnesses, each named at its row and family.  The fixtures and the
tests it has in common with the other shipped tables are word_tables.cpu_tests over this table's record; its own follow.
Nothing here needs a GPU; the device side is tests/test_gpu_arithmetic_mod.py."""
import arithmetic_mod_model as model
from proof_protocol_decoder_amd import arithmetic_mod as am
from word_tables import MODULAR, cpu_tests

globals().update(cpu_tests(MODULAR))


def test_a_padding_row_is_zero_but_for_z_and_the_carry_offsets():
    row = model.cells(model.honest(*model.PADDING[0]))
    offsets = {model.CARRY + model.CARRY_BITS * k + 20 for k in range(31)}
    assert {c for c, v in enumerate(row) if v} == {model.Z} | offsets and all(row[c] == 1 for c in offsets)


def test_both_carry_extremes_are_reached_and_fit():
    """AIRS.md: each side's own carry is at most 16 (2^16 - 1) + 1, so |c_k| < 2^20"""
    assert 16 * (model.B - 1) + 1 < model.CARRY_OFFSET == 1 << (model.CARRY_BITS - 1)
    lo = model.honest(model.MULMOD, *model.MOST_NEGATIVE, 1)["signed_carry"]
    hi = model.honest(model.MULMOD, *model.MOST_POSITIVE, 1)["signed_carry"]
    assert min(lo) == -0xEFFF1 and max(hi) == hi[15] == 0xFFFEF
    for op in model.edge_ops_full() + model.random_ops(1500, 0xCA45):
        c = model.honest(*op)["signed_carry"]
        assert -0xEFFF1 <= min(c) and max(c) <= 0xFFFEF, op


def test_the_model_rows_state_the_evm_operations():
    """the model against the statement itself: (a + b) % m and (a * b) % m, zero for m = 0"""
    for op, a, b, m, e in model.edge_ops_full():
        w = model.honest(op, a, b, m, e)
        if op not in (model.ADDMOD, model.MULMOD):
            assert model.word(w["resl"]) == 0 and w["g"] == 0
            continue
        u = a + b if op == model.ADDMOD else a * b
        assert model.word(w["resl"]) == (u % m if m else 0)
        assert model.word(w["ql"]) * (m if m else 1 << 256) + w["rb"] == u and (w["rb"] < m or not m)


def test_the_wrapped_sum_breaks_the_first_column_above_the_low_half(program):
    """ADDMOD from (a + b) mod 2^256: columns 0 .. 15 add up, column 16 is where the missing 2^256 shows"""
    row = model.forged(model.CATALOGUE[0])
    broken = [k for k, v in enumerate(program.evaluate(row, row)) if v]
    assert broken == [am.first_index("product") + 16]
