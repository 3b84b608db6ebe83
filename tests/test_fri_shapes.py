"""Host side of the whole-proof tests away from (cap_height, final_poly_bits) = (4, 5): the Python statement of a proof's
shape (fri_shape_cases.py) against the table measured from the oracle and against the oracle itself, and the product's CPU
verifier (csrc/verifier.cpp, which derives the same layout as the prover) on the oracle's proofs of every case.  No GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

from builtin_airs import product_verify
from fri_shape_cases import (ARITY_BITS, CASES, CHAINS, case_id, chain_config, chain_id, final_len, flip_words, layout, n_layers,
                              proof_words)

CASE_PARAMS = [pytest.param(c, id=case_id(c)) for c, _, _, _ in CASES]


def configs(oracle, c):
    """the oracle's configuration of a case; the product's has the same first ten fields (product_verify copies them)"""
    return oracle.make_cfg(c.log_n, c.n_cols, n_const=c.n_const, deg_pow=c.deg_pow, rate_bits=c.rate_bits, cap_height=c.cap_height,
                           num_queries=c.num_queries, pow_bits=c.pow_bits, arity_bits=ARITY_BITS, final_poly_bits=c.final_poly_bits)


def case_seeds(c):
    return 0x5EED000000000000 + 100 * c.log_n + 10 * c.cap_height + c.final_poly_bits, 77


@functools.lru_cache(maxsize=None)
def _oracle_proof(c):
    from oracle import pyoracle as oracle
    seed, const_seed = case_seeds(c)
    cfg = configs(oracle, c)
    consts = oracle.synth_constants(const_seed, c.log_n, c.n_const) if c.n_const else None
    cc = oracle.Committed.from_values(consts, c.rate_bits, c.cap_height) if c.n_const else None
    tr = oracle.synth_trace(seed, cfg, consts)
    tc = oracle.Committed.from_values(tr, c.rate_bits, c.cap_height)
    ch = oracle.PyChallenger()
    if cc is not None:
        ch.observe(cc.cap())
    ch.observe(tc.cap())
    ctl = np.array([ch.challenge() for _ in range(4)], dtype=np.uint64)
    chv = ch.clone()
    proof = oracle.stark_prove(cfg, tr, ctl, ch, cc, tc)
    proof.setflags(write=False)
    return cfg, proof, ctl, chv, (cc.cap() if cc is not None else None)


def oracle_proof(oracle, c):
    """The oracle's proof of the case's seeded synthetic table, computed once per process and shared (read-only) ->
    (cfg, proof words, the four lookup challenges, the challenger as the oracle's verifier needs it, the constants' cap)"""
    cfg, proof, ctl, chv, const_cap = _oracle_proof(c)
    return cfg, proof, ctl, chv.clone(), const_cap


def check_product_verifier(cfg, c, proof, const_cap):
    """the product's CPU verifier accepts `proof` and notices one flipped bit in each of flip_words(c)"""
    import proof_protocol_decoder_amd as pkg
    assert product_verify(cfg, 0, proof, const_cap) == 0, pkg.lib().bp_last_error()
    for k, (name, word) in enumerate(flip_words(c)):
        bad = np.array(proof, dtype=np.uint64)
        bad[word] ^= np.uint64(1 << (3 + 11 * k))
        assert product_verify(cfg, 0, bad, const_cap) == -5, "a flipped bit in the %s (word %d) went unnoticed" % (name, word)


def test_shape_formula_matches_the_table():
    """n_layers, final_len and the proof length in Python integers against what was measured from the oracle, and the
    branch each case is in the table for."""
    for c, layers, words, _ in CASES:
        assert (n_layers(c), proof_words(c)) == (layers, words), c
        assert final_len(c) == 1 << (c.log_n - 4 * layers)
    by_id = {case_id(c): c for c, _, _, _ in CASES}
    assert len(by_id) == len(CASES) == 15
    assert layout(by_id["logn4_C8_K0_cap5_fpb5"])["depth0"] == 0 and layout(by_id["logn5_C9_K0_cap6_fpb0"])["depth0"] == 0
    assert layout(by_id["logn8_C16_K0_cap1_fpb0"])["layer_depths"] == [4, 0]        # the last layer's tree is its cap
    assert layout(by_id["logn4_C8_K0_cap0_fpb0"])["layer_depths"] == [1]            # a tree of two leaves
    assert final_len(by_id["logn14_C8_K0_cap8_fpb5"]) == 1024 and final_len(by_id["logn13_C8_K0_cap7_fpb8"]) == 512
    # the cap clause and the arity clause each stop some case on their own, with the other two still allowing a fold (at
    # (4, 5) neither ever does), and the final-polynomial clause is what stops others
    alone, first = set(), False
    for c, layers, _, _ in CASES:
        d = c.log_n - 4 * layers
        clauses = (d > c.final_poly_bits, d + c.rate_bits >= c.cap_height + 4, d >= 4)
        first = first or not clauses[0]
        if sum(clauses) == 2:
            alone.add(clauses.index(False))
    assert alone == {1, 2} and first


def test_longest_final_polynomial_of_any_accepted_configuration():
    """What check_cfg's comment states: over every (log_n, rate_bits, cap_height, final_poly_bits) it accepts, the last FRI
    layer has at most 2^11 points and the final polynomial at most 2^10 coefficients -- far inside the prover's mailbox."""
    from fri_shape_cases import Case
    worst_points = worst_len = 0
    for rate_bits, deg_pow in ((1, 1), (3, 3)):
        for log_n in range(4, 31 - rate_bits):
            for cap in range(0, 9):
                if log_n + rate_bits < cap:
                    continue
                for fpb in range(0, 9):
                    c = Case(log_n, 8, 0, deg_pow, rate_bits, 1, 0, cap, fpb)
                    if n_layers(c) > 8:
                        continue
                    worst_len = max(worst_len, final_len(c))
                    worst_points = max(worst_points, final_len(c) << rate_bits)
    assert (worst_len, worst_points) == (1 << 10, 1 << 11)


@pytest.mark.parametrize("c", CASE_PARAMS)
def test_oracle_shape_and_self_check(oracle, c):
    """The oracle's own layer count and proof length equal the formula's, its header says so, its verifier accepts its proof
    and rejects the five flips: the reference the other tests compare with is sound at this shape."""
    cfg, proof, ctl, chv, const_cap = oracle_proof(oracle, c)
    L = layout(c)
    assert oracle.lib().orc_cfg_n_layers(C.byref(cfg)) == L["n_layers"] and oracle.lib().orc_proof_words(C.byref(cfg)) == L["total"]
    assert proof.size == L["total"] and (int(proof[9]), int(proof[10])) == (L["n_layers"], L["final_len"])
    assert oracle.stark_verify(cfg, proof, ctl, chv, const_cap) == 0
    for name, word in flip_words(c):
        bad = np.array(proof, dtype=np.uint64)
        bad[word] ^= np.uint64(1 << 5)
        ch = oracle.PyChallenger()
        if const_cap is not None:
            ch.observe(const_cap)
        ch.observe(bad[L["trace_cap"]:L["trace_cap"] + L["cap_words"]])
        ctl2 = np.array([ch.challenge() for _ in range(4)], dtype=np.uint64)
        assert oracle.stark_verify(cfg, bad, ctl2, ch, const_cap) != 0, name


@pytest.mark.parametrize("c", CASE_PARAMS)
def test_product_cpu_verifier_accepts_oracle_proofs_and_rejects_flips(oracle, c):
    """bp_stark_verify_air on the oracle's proof of every case: accepted, and one flipped bit in a trace-cap word, a FRI-cap
    word, a final-polynomial word, the proof-of-work word and the last word of the last query is each rejected (BP_ERR_VERIFY)."""
    cfg, proof, _, _, const_cap = oracle_proof(oracle, c)
    check_product_verifier(cfg, c, proof, const_cap)
    # under the neighbouring cap height the same bytes are not a proof (another layout: refused, not read past its end)
    other = cfg.__class__.from_buffer_copy(cfg)
    other.cap_height = c.cap_height - 1 if c.cap_height else 1
    assert product_verify(other, 0, proof, const_cap) != 0


def test_l0_bounds_are_refused_by_the_cpu_verifier_entry(oracle):
    """cap_height = 9, final_poly_bits = 9 and a cap taller than the tree (log_n + rate_bits < cap_height) are invalid input
    (-2) to bp_stark_verify_air, whatever the proof bytes are; the largest accepted values are not."""
    import proof_protocol_decoder_amd as pkg
    L = pkg.lib()
    junk = np.zeros(64, dtype=np.uint64)
    for kw, word in ((dict(cap_height=9), b"cap_height"), (dict(final_poly_bits=9), b"final_poly_bits"),
                     (dict(log_n=4, cap_height=6), b"log_n"), (dict(log_n=6, cap_height=8), b"log_n")):
        cfg = oracle.make_cfg(**dict(dict(log_n=8, n_cols=16, num_queries=5, pow_bits=6), **kw))
        assert product_verify(cfg, 0, junk) == -2, kw
        assert word in L.bp_last_error(), (kw, L.bp_last_error())
    for kw in (dict(cap_height=8), dict(final_poly_bits=8), dict(log_n=4, cap_height=5), dict(log_n=7, cap_height=8)):
        cfg = oracle.make_cfg(**dict(dict(log_n=8, n_cols=16, num_queries=5, pow_bits=6), **kw))
        assert product_verify(cfg, 0, junk) == -5 and b"bytes" in L.bp_last_error(), kw      # accepted shape, wrong length


@pytest.mark.parametrize("ch", CHAINS, ids=chain_id)
def test_product_cpu_verifier_accepts_oracle_chains(oracle, ch):
    """bp_verify_block_proof / bp_verify_proof (host code: the recursion shape's layout at this cap height and
    final-polynomial bound) on the oracle's transaction, aggregation and block proofs: accepted, a flipped bit in the last
    Merkle path word, in a cap and in the final polynomial rejected."""
    from pg_common import ir_words
    from proof_protocol_decoder_amd import proof_gen as pg
    cfg, log_n = chain_config(ch)
    st = oracle.PgState(**cfg)
    t0 = st.txn(ir_words(7, 0, 0x5EED0001, log_n=log_n))
    root1 = tuple(int(x) for x in t0[4 + 84 + 8:4 + 84 + 12])
    t1 = st.txn(ir_words(7, 1, 0x5EED0002, root_before=root1, gas=(121, 150), log_n=log_n))
    agg = st.agg(t0, False, t1, False)
    blk = st.block(None, agg)
    assert all(st.verify(p) == 0 for p in (t0, t1, agg, blk))
    b = pg.ProverStateBuilder()
    for t, name in enumerate(pg.TABLES):
        getattr(b, "set_%s_circuit_size" % name)(range(cfg["table_log_lo"][t], cfg["table_log_hi"][t]))
    b.set(**{k: v for k, v in cfg.items() if not k.startswith("table_")})
    v = pg.VerifierState.from_caps(b.cfg, st.circuit_caps().reshape(-1))
    v.verify(blk.tobytes())
    for p in (t0, t1, agg):
        v.verify_any(p.tobytes())
    first = 4 + 30 + 16                  # the block proof's STARK proof: container header, 30 public inputs, proof header
    cap_words = 4 << cfg["stark_cap_height"]
    for word in (first + 1, first + 3 * cap_words - 1, blk.size // 2, blk.size - 1):
        bad = blk.copy()
        bad[word] ^= np.uint64(1 << 13)
        with pytest.raises(pg.ProofGenError) as e:
            v.verify(bad.tobytes())
        assert e.value.code == -5, word
