"""The division table on the GPU: the witness kernel (csrc/arithmetic_div.hip) against the independent row model of
tests/arithmetic_div_model.py word for word, then the shipped program through the run-time stack -- the device checker,
the prover and the verifier, the port's running products, and table sets in which a caller's table looks divisions up.
Everything is exact.  The fixtures and the tests it has in common with the other shipped tables are word_tables.gpu_tests over
this table's record; the story of 7 / 2 is its own.  CPU side: tests/test_arithmetic_div.py."""
import arithmetic_div_model as model
from word_tables import DIVISION, gpu_tests, one_claim, proves_and_verifies, refused_by_the_pre_flight_the_prover_and_the_verifier, renamed

globals().update(renamed(gpu_tests(DIVISION), test_a_callers_table_looks_the_operations_up="test_a_callers_table_looks_divisions_up"))


def seven_by_two(bpg, reg, exposed, res):
    """the division table's row 20 (a padding row of the edge list) replaced by 7 / 2, the only claim of the looking table"""
    return one_claim(bpg, DIVISION, reg, (model.DIV, 7, 2), exposed, res, 0xD176)


def test_seven_by_two_is_three(bpg, reg):
    tables, traces, _ = seven_by_two(bpg, reg, 1, 3)
    proves_and_verifies(bpg, tables, traces)


def test_a_claim_that_seven_by_two_is_four_is_refused(bpg, reg):
    tables, traces, row = seven_by_two(bpg, reg, 1, 4)
    refused_by_the_pre_flight_the_prover_and_the_verifier(bpg, tables, traces, row, DIVISION.claim_row)


def test_a_division_that_is_not_exposed_cannot_be_looked_up(bpg, reg):
    tables, traces, row = seven_by_two(bpg, reg, 0, 3)
    refused_by_the_pre_flight_the_prover_and_the_verifier(bpg, tables, traces, row, -1)
