"""The division table on the CPU: the shipped program (proof_protocol_decoder_amd/arithmetic_div.py) against the
independent row model of tests/arithmetic_div_model.py -- the column maps, Builder.evaluate over Python integers, the
library's host checker -- and a catalogue of wrong witnesses, each named at its row and family.  The fixtures and the
tests it has in common with the other shipped tables are word_tables.cpu_tests over this table's record; its own follow.
Nothing here needs a GPU; the device side is tests/test_gpu_arithmetic_div.py."""
import arithmetic_div_model as model
from word_tables import DIVISION, cpu_tests, renamed

globals().update(renamed(cpu_tests(DIVISION),
                         test_the_layout_entry_refuses_a_short_or_null_buffer="test_the_layout_entry_refuses_a_short_buffer",
                         test_unpack_row_and_pack_inputs_give_back_the_operations="test_unpack_row_and_pack_inputs_give_back_divmod"))


def test_the_largest_carry_is_reached_and_fits():
    w = model.honest(model.DIV, *model.LARGEST_CARRY, 1)
    assert max(w["carry"]) == w["carry"][7] == 0x7FFF7 and 1 << 18 <= 0x7FFF7 < 1 << model.CARRY_BITS
    # the bound in include/bpg.h: at most eight products that are not zero in a column
    assert 8 * (model.B - 1) + 1 < 1 << model.CARRY_BITS
    for op in model.edge_ops_full() + model.random_ops(2000, 0xCA44):
        w = model.honest(*op)
        assert max(w["carry"]) <= 0x7FFF7, op
