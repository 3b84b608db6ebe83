"""AIR 2 (logic: one AND / OR / XOR of two 256-bit words per row) on the CPU: the oracle's witness against Python's big
integers, its constraint list against the witness, and its proofs against the PRODUCT's CPU verifier (csrc/air.hpp
instantiated over the extension field) -- two independent statements of the same 524 constraints (the oracle selects
one polynomial per operation, the product folds them into p (a + b) + q ab), cross-checked before any GPU is
involved.  The record of the AIR and the shared test bodies: tests/builtin_airs.py; GPU side:
tests/test_gpu_logic_air.py."""
import ctypes as C

import numpy as np
import pytest

import builtin_airs as ba
from builtin_airs import logic as air

COL_OP, COL_IN0, COL_IN1, COL_RES, N_COLS = air.COL_OP, air.COL_IN0, air.COL_IN1, air.COL_RES, air.n_cols


def test_trace_rows_are_the_operations_on_python_integers(oracle):
    log_n = 6
    inp = air.random_inputs(1 << log_n, 7)
    # edge operands: all zero, all one, equal, complementary
    ones = np.uint64(0xFFFFFFFFFFFFFFFF)
    for r, (op, a, b) in enumerate([(1, 0, 0), (2, ones, ones), (3, ones, ones), (3, ones, 0), (1, ones, 0), (0, ones, ones)]):
        inp[r] = [op] + [a] * 4 + [b] * 4
    t = oracle.logic_trace(log_n, inputs=inp)
    assert t.shape == (N_COLS, 64) and (t[:COL_RES] <= 1).all() and (t[COL_RES:] < np.uint64(1 << 32)).all()
    for r in range(64):
        op = int(inp[r, 0])
        a = sum(int(inp[r, 1 + w]) << (64 * w) for w in range(4))
        b = sum(int(inp[r, 5 + w]) << (64 * w) for w in range(4))
        assert air.word_of(t, r, COL_IN0) == a and air.word_of(t, r, COL_IN1) == b
        assert [int(t[COL_OP + i, r]) for i in range(3)] == [int(op == 1), int(op == 2), int(op == 3)]
        assert air.result_of(t, r) == air.OPS[op](a, b), (r, op)
    # the seeded witness draws all four codes and is reproducible
    s1, s2 = oracle.logic_trace(8, seed=0xABCD), oracle.logic_trace(8, seed=0xABCD)
    assert (s1 == s2).all() and (oracle.logic_trace(8, seed=0xABCE) != s1).any()
    codes = s1[COL_OP] + 2 * s1[COL_OP + 1] + 3 * s1[COL_OP + 2]
    assert set(int(c) for c in codes) == {0, 1, 2, 3}
    for r in range(0, 256, 17):
        assert air.result_of(s1, r) == air.OPS[int(codes[r])](air.word_of(s1, r, COL_IN0), air.word_of(s1, r, COL_IN1))


@pytest.mark.parametrize("log_n", [5, 8])
def test_oracle_proof_is_accepted_by_both_verifiers_and_tampering_is_not(oracle, log_n):
    ba.check_proof_is_accepted_and_tampering_is_not(oracle, air, log_n, oracle.logic_trace(log_n, seed=0xFEED + log_n))


@pytest.mark.parametrize("brk", air.breaks, ids=[b.label for b in air.breaks])
def test_a_witness_that_breaks_one_family_yields_a_rejected_proof(oracle, brk):
    ba.check_break_yields_a_rejected_proof(oracle, air, brk)


def test_air_registry_describes_the_logic_air():
    import proof_protocol_decoder_amd as pkg
    ba.check_registry_describes(air)
    # a table of the wrong width is refused
    cfg = pkg.ops.stark_cfg(6, 523)
    assert pkg.lib().bp_stark_verify_air(2, C.byref(cfg), None, b"\0" * 8, 8) != 0
