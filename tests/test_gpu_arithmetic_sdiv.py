"""The signed table on the GPU: the witness kernel (csrc/arithmetic_sdiv.hip) against the independent row model of
tests/arithmetic_sdiv_model.py word for word, then the shipped program through the run-time stack -- the device checker,
the prover and the verifier, the port's running products, and table sets in which a caller's table looks signed
divisions up.  Everything is exact, at 2^5 rows throughout.  The fixtures and the tests it has in common with the other
shipped tables are word_tables.gpu_tests over this table's record; the stories of the classic mistakes are its own.  CPU
side: tests/test_arithmetic_sdiv.py."""
import pytest

import arithmetic_sdiv_model as model
from word_tables import SIGNED, gpu_tests, one_claim, proves_and_verifies, refused_by_the_pre_flight_the_prover_and_the_verifier

globals().update(gpu_tests(SIGNED))

n_ = model.to_word
# one looking table claims one row, the edge list's padding row SIGNED.claim_row with nothing else exposed: (operation, the
# honest result, the classic wrong one)
STORIES = {"sdiv_truncates": ((model.SDIV, n_(-7), 2), n_(-3), n_(-4)),
           "smod_has_the_sign_of_x": ((model.SMOD, n_(-7), 2), n_(-1), 1),
           "sdiv_of_the_most_negative_word_by_minus_one": ((model.SDIV, 1 << 255, n_(-1)), 1 << 255, 0),
           "sdiv_by_zero": ((model.SDIV, 5, 0), 0, None)}
for _operation, _honest, _ in STORIES.values():
    assert model.statement(*_operation) == _honest


@pytest.mark.parametrize("story", STORIES)
def test_an_honest_claim_is_accepted(bpg, reg, story):
    operation, honest, _ = STORIES[story]
    tables, traces, _ = one_claim(bpg, SIGNED, reg, operation, 1, honest, 0x5D76)
    proves_and_verifies(bpg, tables, traces)


@pytest.mark.parametrize("story", [s for s in STORIES if STORIES[s][2] is not None])
def test_a_wrong_claim_is_refused(bpg, reg, story):
    """the floor for the truncation, the remainder with the divisor's sign, 0 for the quotient 2^255"""
    operation, _, wrong = STORIES[story]
    tables, traces, row = one_claim(bpg, SIGNED, reg, operation, 1, wrong, 0x5D77)
    refused_by_the_pre_flight_the_prover_and_the_verifier(bpg, tables, traces, row, SIGNED.claim_row)


def test_an_operation_that_is_not_exposed_cannot_be_looked_up(bpg, reg):
    operation, honest, _ = STORIES["sdiv_truncates"]
    tables, traces, row = one_claim(bpg, SIGNED, reg, operation, 0, honest, 0x5D78)
    refused_by_the_pre_flight_the_prover_and_the_verifier(bpg, tables, traces, row, -1)
