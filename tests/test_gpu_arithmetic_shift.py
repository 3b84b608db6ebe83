"""The shift table on the GPU: the witness kernel (csrc/arithmetic_shift.hip) against the independent row model of
tests/arithmetic_shift_model.py word for word, then the shipped program through the run-time stack -- the device checker,
the prover and the verifier, the port's running products, and table sets in which a caller's table looks shifts up.
Everything is exact.  The fixtures and the tests it has in common with the other shipped tables are
word_tables.gpu_tests over this table's record; the stories of the masked count are its own.  CPU side:
tests/test_arithmetic_shift.py."""
import arithmetic_shift_model as model
from word_tables import SHIFT, gpu_tests, one_claim, proves_and_verifies, refused_by_the_pre_flight_the_prover_and_the_verifier, renamed

globals().update(renamed(gpu_tests(SHIFT), test_a_callers_table_looks_the_operations_up="test_a_callers_table_looks_shifts_up"))

# one looking table claims one row, the edge list's padding row SHIFT.claim_row with nothing else exposed
X_ = model.G2                                  # SHL(256, x) = 0, and x itself if only the count's low byte were read
NEG = model.G1                                 # a negative word: SAR(2^16 + 5, x) is all ones, SAR(5, x) is not
assert model.statement(model.SHL, 256, X_) == 0 and model.statement(model.SHL, 256 & 0xFF, X_) == X_
assert model.statement(model.SAR, model.LIMB_ONE, NEG) == model.MAX != model.statement(model.SAR, 5, NEG)


def test_a_shift_by_256_is_zero(bpg, reg):
    tables, traces, _ = one_claim(bpg, SHIFT, reg, (model.SHL, 256, X_), 1, 0, 0x5F76)
    proves_and_verifies(bpg, tables, traces)


def test_a_claim_of_the_masked_counts_answer_is_refused(bpg, reg):
    tables, traces, row = one_claim(bpg, SHIFT, reg, (model.SHL, 256, X_), 1, X_, 0x5F76)
    refused_by_the_pre_flight_the_prover_and_the_verifier(bpg, tables, traces, row, SHIFT.claim_row)


def test_sar_past_the_word_is_the_sign(bpg, reg):
    tables, traces, _ = one_claim(bpg, SHIFT, reg, (model.SAR, model.LIMB_ONE, NEG), 1, model.MAX, 0x5F77)
    proves_and_verifies(bpg, tables, traces)


def test_a_claim_of_sar_by_the_masked_count_is_refused(bpg, reg):
    tables, traces, row = one_claim(bpg, SHIFT, reg, (model.SAR, model.LIMB_ONE, NEG), 1, model.statement(model.SAR, 5, NEG), 0x5F77)
    refused_by_the_pre_flight_the_prover_and_the_verifier(bpg, tables, traces, row, SHIFT.claim_row)


def test_an_operation_that_is_not_exposed_cannot_be_looked_up(bpg, reg):
    tables, traces, row = one_claim(bpg, SHIFT, reg, (model.SHL, 256, X_), 0, 0, 0x5F76)
    refused_by_the_pre_flight_the_prover_and_the_verifier(bpg, tables, traces, row, -1)
