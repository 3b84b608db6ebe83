"""The modular table on the GPU: the witness kernel (csrc/arithmetic_mod.hip) against the independent row model of
tests/arithmetic_mod_model.py word for word, then the shipped program through the run-time stack -- the device checker,
the prover and the verifier, the port's running products, and table sets in which a caller's table looks modular
operations up.  Everything is exact.  The fixtures and the tests it has in common with the other shipped tables are
word_tables.gpu_tests over this table's record; the story of the sum that wraps is its own.  CPU side:
tests/test_arithmetic_mod.py."""
import arithmetic_mod_model as model
from word_tables import MODULAR, gpu_tests, one_claim, proves_and_verifies, refused_by_the_pre_flight_the_prover_and_the_verifier, renamed

globals().update(renamed(gpu_tests(MODULAR), test_a_callers_table_looks_the_operations_up="test_a_callers_table_looks_modular_operations_up"))

A_, B_ = (1 << 256) - 3, 10          # a + b = 2^256 + 7: (a + b) mod 9 = 5, but ((a + b) mod 2^256) mod 9 = 7
assert (A_ + B_) % 9 == 5 and ((A_ + B_) % (1 << 256)) % 9 == 7


def one_addmod(bpg, reg, exposed, res):
    """the modular table's row 21 (a padding row of the edge list) replaced by ADDMOD(2^256 - 3, 10, 9), the only claim
    of the looking table"""
    return one_claim(bpg, MODULAR, reg, (model.ADDMOD, A_, B_, 9), exposed, res, 0xA076)


def test_the_sum_is_reduced_over_the_integers(bpg, reg):
    tables, traces, _ = one_addmod(bpg, reg, 1, 5)
    proves_and_verifies(bpg, tables, traces)


def test_a_claim_of_the_wrapped_sums_answer_is_refused(bpg, reg):
    tables, traces, row = one_addmod(bpg, reg, 1, 7)
    refused_by_the_pre_flight_the_prover_and_the_verifier(bpg, tables, traces, row, MODULAR.claim_row)


def test_an_operation_that_is_not_exposed_cannot_be_looked_up(bpg, reg):
    tables, traces, row = one_addmod(bpg, reg, 0, 5)
    refused_by_the_pre_flight_the_prover_and_the_verifier(bpg, tables, traces, row, -1)
