"""AIR 4 (ADD / SUB / LT / GT on 256-bit words, sixteen 16-bit limbs, one carry chain) on the CPU: the oracle's witness
against Python's integers, its constraint list against the witness, and its proofs against the PRODUCT's CPU verifier
(csrc/air.hpp over the extension field) -- two independent statements of the same 294 constraints (the oracle writes
one limb equation per operation, the product collects the coefficients of x, y and z).  The record of the AIR and the
shared test bodies: tests/builtin_airs.py; GPU side: tests/test_gpu_arithmetic_air.py."""
import numpy as np
import pytest

import builtin_airs as ba
from builtin_airs import arithmetic as air

COL_OP, COL_X, COL_Y, COL_Z, COL_RES, N_COLS, M = air.COL_OP, air.COL_X, air.COL_Y, air.COL_Z, air.COL_RES, air.n_cols, air.M


def test_trace_rows_are_the_operations_on_python_integers(oracle):
    log_n = 6
    inp = air.random_inputs(1 << log_n, 21)
    edge = [(1, M - 1, 1), (1, M - 1, M - 1), (2, 0, 1), (2, 5, 5), (3, 7, 7), (3, 0, M - 1), (3, M - 1, 0), (4, 7, 7),
            (4, 1 << 255, (1 << 255) - 1), (4, 0xFFFF, 0x10000), (1, 0xFFFF, 1), (0, M - 1, M - 1), (9, 3, 4)]
    for r, (op, x, y) in enumerate(edge):
        inp[r] = [op] + air.words(x) + air.words(y)
    t = oracle.arithmetic_trace(log_n, inputs=inp)
    assert t.shape == (N_COLS, 64) and (t[COL_X:COL_Z] < np.uint64(1 << 16)).all()
    assert (t[COL_Z:COL_RES + 1] <= 1).all() and (t[:COL_X] <= 1).all()
    for r in range(64):
        op = int(inp[r, 0]) if int(inp[r, 0]) <= 4 else 0
        x = sum(int(inp[r, 1 + w]) << (64 * w) for w in range(4))
        y = sum(int(inp[r, 5 + w]) << (64 * w) for w in range(4))
        air.check_row(t, r, op, x, y)
    s1 = oracle.arithmetic_trace(8, seed=0x1234)
    assert (oracle.arithmetic_trace(8, seed=0x1234) == s1).all() and (oracle.arithmetic_trace(8, seed=0x1235) != s1).any()
    codes = s1[COL_OP] + 2 * s1[COL_OP + 1] + 3 * s1[COL_OP + 2] + 4 * s1[COL_OP + 3]
    assert set(int(c) for c in codes) == {0, 1, 2, 3, 4}
    for r in range(0, 256, 13):
        air.check_row(s1, r, int(codes[r]), air.limbs_word(s1, r, COL_X), air.limbs_word(s1, r, COL_Y))


@pytest.mark.parametrize("log_n", [5, 8])
def test_oracle_proof_is_accepted_by_both_verifiers_and_tampering_is_not(oracle, log_n):
    ba.check_proof_is_accepted_and_tampering_is_not(oracle, air, log_n, oracle.arithmetic_trace(log_n, seed=0xA11CE + log_n))


@pytest.mark.parametrize("brk", air.breaks, ids=[b.label for b in air.breaks])
def test_a_witness_that_breaks_one_family_yields_a_rejected_proof(oracle, brk):
    ba.check_break_yields_a_rejected_proof(oracle, air, brk)


def test_air_registry_describes_the_arithmetic_air():
    ba.check_registry_describes(air)
