"""AIR 5 (byte packing: a big-endian sequence of 1..32 bytes and the 256-bit word it spells) on the CPU: the oracle's
witness against int.from_bytes, its constraint list against the witness, and its proofs against the PRODUCT's CPU
verifier (csrc/air.hpp over the extension field) -- two independent statements of the same 330 constraints (the oracle
writes the value length by length, the product regroups it by byte slot).  The record of the AIR and the shared test
bodies: tests/builtin_airs.py; GPU side: tests/test_gpu_byte_packing_air.py."""
import numpy as np
import pytest

import builtin_airs as ba
from builtin_airs import byte_packing as air

COL_READ, COL_LEN, COL_VAL, N_COLS = air.COL_READ, air.COL_LEN, air.COL_VAL, air.n_cols
BREAKS = [b for b in air.breaks if b.target != ba.CHECKER]


def test_trace_rows_spell_big_endian_words(oracle):
    log_n = 7
    inp = air.random_inputs(1 << log_n, 31)
    for r, ln in enumerate([0, 1, 2, 3, 4, 5, 8, 16, 31, 32, 40]):     # every boundary; 40 is clipped to 32
        inp[r, 1] = ln
    inp[11, 2:] = np.uint64(0xFFFFFFFFFFFFFFFF)
    inp[11, 1] = 32
    t = oracle.byte_packing_trace(log_n, inputs=inp)
    assert t.shape == (N_COLS, 128) and (t[:COL_VAL] <= 1).all() and (t[COL_VAL:] < np.uint64(1 << 32)).all()
    for r in range(128):
        data = b"".join(int(inp[r, 2 + w]).to_bytes(8, "little") for w in range(4))
        air.check_row(t, r, int(inp[r, 0]) & 1, min(int(inp[r, 1]), 32), data)
    s1 = oracle.byte_packing_trace(9, seed=0xB17E)
    assert (oracle.byte_packing_trace(9, seed=0xB17E) == s1).all() and (oracle.byte_packing_trace(9, seed=0xB17F) != s1).any()
    lens = sum(j * s1[COL_LEN + j - 1] for j in range(1, 33))
    assert set(int(x) for x in lens) == set(range(33))                  # every length occurs among 512 seeded rows
    for r in range(0, 512, 29):
        ln = int(lens[r])
        air.check_row(s1, r, int(s1[COL_READ, r]), ln, air.slots_of(s1, r))


@pytest.mark.parametrize("log_n", [5, 9])
def test_oracle_proof_is_accepted_by_both_verifiers_and_tampering_is_not(oracle, log_n):
    ba.check_proof_is_accepted_and_tampering_is_not(oracle, air, log_n, oracle.byte_packing_trace(log_n, seed=0xBEEF00 + log_n))


@pytest.mark.parametrize("brk", BREAKS, ids=[b.label for b in BREAKS])
def test_a_witness_that_breaks_one_family_yields_a_rejected_proof(oracle, brk):
    ba.check_break_yields_a_rejected_proof(oracle, air, brk)


def test_air_registry_describes_the_byte_packing_air():
    ba.check_registry_describes(air)
