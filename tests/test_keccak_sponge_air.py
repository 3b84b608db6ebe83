"""AIR 6 (the absorbing side of Keccak-256: one 136-byte block per row) on the CPU: the rows of a message against
hashlib's Keccak... the oracle's permutation, its witness against the rows, its constraint list against the witness, and
its proofs against the PRODUCT's CPU verifier (csrc/air.hpp over the extension field) -- two independent statements of
the same 2587 constraints (the oracle states pad10*1 as three cases per byte, the product through a running sum of the
length flags).  The record of the AIR and the shared test bodies: tests/builtin_airs.py; GPU side:
tests/test_gpu_keccak_sponge_air.py."""
import numpy as np
import pytest

import builtin_airs as ba
from builtin_airs import keccak_sponge as air

COL_LEN, COL_BLOCK, COL_RATE, COL_CAP, COL_XORED, COL_UPDATED, N_COLS = (air.COL_LEN, air.COL_BLOCK, air.COL_RATE, air.COL_CAP,
                                                                       air.COL_XORED, air.COL_UPDATED, air.n_cols)
MESSAGES, lanes = air.MESSAGES, air.lanes


def test_rows_of_messages_end_in_their_keccak256(oracle):
    """Known answers: the product's and the oracle's row builders agree, chain through the permutation, pad correctly at
    every boundary length, and the last row of a message leaves its Keccak-256 (compact.keccak256, itself pinned by the
    reference's golden MPT roots) in the updated state."""
    from proof_protocol_decoder_amd import compact, proof_gen as pg
    for m in MESSAGES:
        d, r = oracle.keccak_sponge_rows(m)
        d2, r2 = pg.keccak256_sponge_rows(m)
        assert d == d2 == compact.keccak256(m) and r.tolist() == r2
        assert [int(x) for x in r[:, 0]] == [1] * (len(m) // 136) + [2] and int(r[-1, 1]) == len(m) % 136
        assert not r[0, 19:].any()                                   # a message starts from the zero state
        blocks = b"".join(int(w).to_bytes(8, "little") for row in r for w in row[2:19])
        padded = bytearray(m) + b"\x00" * (136 - len(m) % 136)
        padded[len(m)] ^= 0x01
        padded[-1] ^= 0x80
        assert blocks == bytes(padded)
    rows, k, digests = air.rows_of(oracle, MESSAGES, 4)
    t = oracle.keccak_sponge_trace(4, inputs=rows)
    assert t.shape == (N_COLS, 16) and (t[:COL_CAP] <= 1).all() and (t[COL_CAP:] < np.uint64(1 << 32)).all()
    r = 0
    for m, d in zip(MESSAGES, digests):
        n = len(m) // 136 + 1
        last = r + n - 1
        out = lanes(t, last, COL_UPDATED, 4)
        assert b"".join(x.to_bytes(8, "little") for x in out) == d
        for i in range(r, last):                                     # chaining inside the message
            assert lanes(t, i, COL_UPDATED, 25) == [sum(int(t[COL_RATE + 64 * l + z, i + 1]) << z for z in range(64)) for l in range(17)] + \
                [int(t[COL_CAP + 2 * l, i + 1]) | (int(t[COL_CAP + 2 * l + 1, i + 1]) << 32) for l in range(8)]
        assert int(t[COL_LEN + len(m) % 136, last]) == 1 and int(t[COL_LEN:COL_BLOCK, last].sum()) == 1
        r += n
    assert not t[:, k:].any()                                        # the rest: padding rows
    # the (xored rate, capacity) of a row is what its Keccak-f permutation takes in: the link to AIR 1
    inp = lanes(t, 0, COL_XORED, 17) + [int(t[COL_CAP + 2 * l, 0]) | (int(t[COL_CAP + 2 * l + 1, 0]) << 32) for l in range(8)]
    assert lanes(t, 0, COL_UPDATED, 25) == [int(x) for x in oracle.keccak_f(np.array(inp, dtype=np.uint64))]


@pytest.mark.parametrize("seeded", [True, False], ids=["seeded", "messages"])
def test_oracle_proof_is_accepted_by_both_verifiers_and_tampering_is_not(oracle, seeded):
    log_n = 5
    trace = oracle.keccak_sponge_trace(log_n, seed=0x5907) if seeded else oracle.keccak_sponge_trace(log_n, inputs=air.rows_of(oracle, MESSAGES * 2, log_n)[0])
    ba.check_proof_is_accepted_and_tampering_is_not(oracle, air, log_n, trace)


@pytest.mark.parametrize("brk", air.breaks, ids=[b.label for b in air.breaks])
def test_a_witness_that_breaks_one_family_yields_a_rejected_proof(oracle, brk):
    ba.check_break_yields_a_rejected_proof(oracle, air, brk)


def test_air_registry_describes_the_keccak_sponge_air():
    ba.check_registry_describes(air)
