"""AIR 1 (Keccak-f[1600], one round per row) on the CPU: the oracle's permutation against hashlib, its witness
against the permutation, its constraint list against the witness, and its proofs against the PRODUCT's CPU verifier
(csrc/air.hpp instantiated over the extension field) -- two independent statements of the same 2826 constraints,
cross-checked before any GPU is involved.  The record of the AIR (columns, generators, breaks) and the test bodies all
seven AIRs share are in tests/builtin_airs.py; the GPU side of the same AIR is in tests/test_gpu_keccak_air.py."""
import hashlib

import numpy as np
import pytest

import builtin_airs as ba
from builtin_airs import P, keccak as air

COL_STEP, COL_A, COL_C, COL_APP, COL_APP0, COL_APPP = air.COL_STEP, air.COL_A, air.COL_C, air.COL_APP, air.COL_APP0, air.COL_APPP


@pytest.mark.parametrize("msg", [b"", b"abc", b"q" * 135, b"r" * 136, b"The quick brown fox" * 20])
def test_oracle_permutation_reproduces_sha3_256(oracle, msg):
    digest, _ = air.sha3_256_by_hand(oracle.keccak_f, msg)
    assert digest == hashlib.sha3_256(msg).digest()


def test_oracle_permutation_known_answer(oracle):
    # Keccak-f[1600] of the all-zero state (the Keccak team's KeccakF-1600 intermediate values, first two lanes)
    z = oracle.keccak_f(np.zeros(25, dtype=np.uint64))
    assert (int(z[0]), int(z[1])) == (0xF1258F7940E1DDE7, 0x84D5CCF933C0478A)


def test_trace_rows_are_the_rounds_of_the_permutation(oracle):
    """Known answers through the witness: the trace of the sponge blocks of a message ends, 24 rows later, in the
    state whose first four lanes are hashlib's SHA3-256."""
    msg = b"proof-protocol-decoder" * 9          # two blocks
    digest, blocks = air.sha3_256_by_hand(oracle.keccak_f, msg)
    log_n = 6                                     # 64 rows: permutations 0, 1 and 16 rows of a third
    inputs = np.zeros((3, 25), dtype=np.uint64)
    inputs[0], inputs[1] = blocks[0], blocks[1]
    t = oracle.keccak_trace(log_n, inputs=inputs)
    assert t.shape == (2431, 64) and (t < np.uint64(P)).all()
    for p, blk in enumerate(blocks):
        assert (air.lanes_of(t, 24 * p, COL_A) == blk).all()
        out = air.lanes_of(t, 24 * p + 23, COL_APP)
        out[0] = int(t[COL_APPP, 24 * p + 23]) | (int(t[COL_APPP + 1, 24 * p + 23]) << 32)
        assert (out == oracle.keccak_f(blk)).all()
    assert out[:4].astype("<u8").tobytes() == hashlib.sha3_256(msg).digest() == digest
    # one-hot flags, bits are bits, rows chain inside a permutation
    assert (t[COL_STEP:COL_STEP + 24].sum(axis=0) == 1).all()
    assert all(int(t[COL_STEP + r % 24, r]) == 1 for r in range(64))
    assert (t[COL_C:COL_APP] <= 1).all() and (t[COL_APP0:COL_APPP] <= 1).all()
    for r in range(63):
        if r % 24 != 23:
            nxt = air.lanes_of(t, r + 1, COL_A)
            cur = air.lanes_of(t, r, COL_APP)
            cur[0] = int(t[COL_APPP, r]) | (int(t[COL_APPP + 1, r]) << 32)
            assert (nxt == cur).all()


@pytest.mark.parametrize("log_n", [5, 7])
def test_oracle_proof_is_accepted_by_both_verifiers_and_tampering_is_not(oracle, log_n):
    ba.check_proof_is_accepted_and_tampering_is_not(oracle, air, log_n, oracle.keccak_trace(log_n, seed=0xBEEF + log_n))


def test_queries_checked_by_several_threads_report_the_first_failing_query(oracle):
    """stark_verify checks the queries of a proof with >= 16 of them on up to four threads when the process is not busy
    proving; what it reports must be what the sequential loop reports: acceptance, and for a proof with TWO corrupted
    queries the failure of the lower one."""
    import proof_protocol_decoder_amd as pkg
    log_n = 5
    cfg = ba.small_cfg(oracle, air, log_n, num_queries=20)
    trace = oracle.keccak_trace(log_n, seed=0xBEEF)
    proof, ctl, chv = ba.prove(oracle, cfg, trace)
    assert ba.product_verify(cfg, 1, proof) == 0
    # the layout: the query section is the tail of the proof, 20 records of equal length
    q_words = None
    for cand in range(1, proof.size):
        if (proof.size - cand * 20) > 0 and int(proof[proof.size - cand * 20]) < (1 << (log_n + 1)) and cand > 2431:
            q_words = cand
            break
    assert q_words is not None
    bad = proof.copy()
    first = proof.size - 20 * q_words
    bad[first + 13 * q_words + 5] ^= np.uint64(1)       # a trace value of query 13
    bad[first + 6 * q_words + 9] ^= np.uint64(1)        # ... and of query 6
    assert ba.product_verify(cfg, 1, bad) != 0
    assert b"query 6:" in pkg.lib().bp_last_error()


@pytest.mark.parametrize("brk", air.breaks, ids=[b.label for b in air.breaks])
def test_a_witness_that_breaks_one_family_yields_a_rejected_proof(oracle, brk):
    ba.check_break_yields_a_rejected_proof(oracle, air, brk)


def test_air_registry_describes_both_airs():
    import proof_protocol_decoder_amd as pkg
    assert pkg.lib().bp_air_count() == 9
    fams = ba.check_registry_describes(air)
    assert max(deg for _, _, _, deg in fams) == 3
    s = pkg.ops.air_describe(0, n_cols=135, n_const=82, deg_pow=3)
    assert s.name == b"synthetic" and (s.fixed_n_cols, s.n_cols, s.degree, s.n_air_constraints) == (0, 135, 9, 99)
    from proof_protocol_decoder_amd._lib import BpgError
    with pytest.raises(BpgError):
        pkg.ops.air_describe(99)


def test_oracle_txn_with_the_keccak_flag_differs_only_through_table_3(oracle):
    """The IR flag 0x100 (Keccak table = AIR 1) in the oracle's generate_txn_proof: accepted, different from the
    all-synthetic proof of the same IR, refused when table 3 is not 2431 columns wide."""
    from pg_common import LOG_N, SMALL, WIDTH, ir_words
    st = oracle.PgState(**SMALL)
    width = list(WIDTH)
    width[3] = 2431
    iw = ir_words(5, 0, 0x5EED0042, width=tuple(width))
    plain = st.txn(iw)
    iw[1] = 0x101
    flagged = st.txn(iw)
    assert plain.shape == flagged.shape and (plain != flagged).any()
    assert st.verify(flagged) == 0
    bad = ir_words(5, 0, 0x5EED0042)
    bad[1] = 0x101
    with pytest.raises(Exception):
        st.txn(bad)
