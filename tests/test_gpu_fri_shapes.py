"""Whole proofs on the GPU away from (cap_height, final_poly_bits) = (4, 5), the one point every other whole-proof test runs
at: the cases of fri_shape_cases.py (root caps, caps that are the leaf level, the three clauses of the layer count, final
polynomials of 1 to 1024 coefficients, 2-leaf layer trees) against the oracle word for word and against both verifiers; a
built-in table with a lookup side, a registered program, and transaction / aggregation / block chains (whose recursion
chains are the lock-step batches) at other caps and bounds.  Everything is exact.  Host side: tests/test_fri_shapes.py."""
import numpy as np
import pytest

import air_program_cases as programs
from builtin_airs import arithmetic, memory, product_verify, prove
from fri_shape_cases import ARITY_BITS, CHAINS, chain_config, chain_id, layout
from test_fri_shapes import CASE_PARAMS, case_seeds, check_product_verifier, oracle_proof

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("loaded", [0, 1], ids=["alone", "loaded"])
@pytest.mark.parametrize("c", CASE_PARAMS)
def test_whole_proof_matches_the_oracle_and_both_verifiers(bpg, oracle, c, loaded):
    """bp_stark_prove_synthetic == the oracle's proof in every word, in the forms the library takes alone and under load; the
    header names the layer count and final length of the Python formula; the oracle's verifier and the product's CPU verifier
    accept the device's proof, and the latter rejects it after one flipped bit in a trace-cap word, a FRI-cap word, a
    final-polynomial word, the proof-of-work word and the last word of the last query."""
    cfg, want, ctl, chv, const_cap = oracle_proof(oracle, c)
    seed, const_seed = case_seeds(c)
    pc = bpg.ops.stark_cfg(c.log_n, c.n_cols, n_const=c.n_const, deg_pow=c.deg_pow, rate_bits=c.rate_bits, cap_height=c.cap_height,
                           num_queries=c.num_queries, pow_bits=c.pow_bits, arity_bits=ARITY_BITS, final_poly_bits=c.final_poly_bits)
    with bpg.ops.tuned(assume_loaded=loaded):
        got = bpg.ops.stark_prove_synthetic(pc, seed, const_seed)
    L = layout(c)
    assert got.shape == want.shape == (L["total"],)
    assert (int(got[9]), int(got[10])) == (L["n_layers"], L["final_len"])
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "first mismatch at word %d of %d (queries start at %d)" % (bad[0], want.size, L["queries"])
    assert oracle.stark_verify(cfg, got, ctl, chv, const_cap) == 0
    check_product_verifier(pc, c, got, const_cap)


@pytest.mark.parametrize("cap,fpb", [(0, 0), (8, 2)])
def test_table_with_a_lookup_side(bpg, oracle, cap, fpb):
    """The memory table (AIR 3: two auxiliary columns of its lookup side, opened at 1 as well) through bp_stark_prove_air at
    2^7 rows -- the smallest height a cap of 256 entries fits, where it is the leaf level of all three trees: the oracle's
    proof word for word, accepted by both verifiers, a flipped bit rejected."""
    log_n, nq, pb = 7, 6, 6
    cfg = oracle.make_cfg(log_n, memory.n_cols, num_queries=nq, pow_bits=pb, cap_height=cap, final_poly_bits=fpb, air_id=memory.id)
    want, ctl, chv = prove(oracle, cfg, oracle.air_trace(memory.id, log_n, seed=memory.gpu_seed))
    pc = bpg.ops.stark_cfg(log_n, memory.n_cols, num_queries=nq, pow_bits=pb, cap_height=cap, final_poly_bits=fpb)
    got = bpg.ops.stark_prove_air(memory.id, pc, memory.gpu_seed)
    assert got.shape == want.shape and int(got[14]) == memory.id
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "first mismatch at word %d of %d" % (bad[0], want.size)
    assert oracle.stark_verify(cfg, got, ctl, chv, None) == 0
    assert product_verify(pc, memory.id, got) == 0
    for word in (16 + 1, got.size // 2, got.size - 1):
        flipped = got.copy()
        flipped[word] ^= np.uint64(1 << 21)
        assert product_verify(pc, memory.id, flipped) == -5, word


def test_registered_program_with_root_caps(bpg, oracle):
    """A registered program (AIR 4's transcription) through bp_stark_prove_trace and bp_stark_verify_air at (0, 0): the proof
    is the built-in's -- which is the oracle's -- in every word but the id in header word 14, verifies under its id only, and
    stops verifying after a flipped bit."""
    log_n, nq, pb = 5, 6, 6
    reg = programs.register(programs.arithmetic_program())
    pc = programs.cfg_for(arithmetic.id, log_n, num_queries=nq, pow_bits=pb, cap_height=0, final_poly_bits=0)
    cfg = oracle.make_cfg(log_n, arithmetic.n_cols, num_queries=nq, pow_bits=pb, cap_height=0, final_poly_bits=0, air_id=arithmetic.id)
    want, ctl, chv = prove(oracle, cfg, oracle.air_trace(arithmetic.id, log_n, seed=arithmetic.gpu_seed))
    trace = bpg.ops.air_trace(arithmetic.id, log_n, seed=arithmetic.gpu_seed)
    built_in = bpg.ops.stark_prove_trace(arithmetic.id, pc, trace)
    got = bpg.ops.stark_prove_trace(reg, pc, trace)
    assert built_in.shape == want.shape and (built_in == want).all()
    assert (int(got[9]), int(got[10]), int(got[14])) == (1, 2, reg)
    assert np.nonzero(got != want)[0].tolist() == [14]
    assert programs.verify(reg, pc, got) == 0
    assert programs.verify(arithmetic.id, pc, got) == -5
    for word in (16 + 2, got.size // 2, got.size - 1):
        flipped = got.copy()
        flipped[word] ^= np.uint64(1 << 33)
        assert programs.verify(reg, pc, flipped) == -5, word


@pytest.mark.parametrize("ch", CHAINS, ids=chain_id)
def test_txn_agg_block_chain_matches_the_oracle(bpg, oracle, ch):
    """Two transactions, their aggregation and the block proof at another cap height and final-polynomial bound: every
    container equals oracle.PgState's byte for byte (a transaction's seven recursion chains are proven as lock-step batches:
    the only B > 1 at these shapes), bp_verify_block_proof / bp_verify_proof accept them -- in the prover state's own verifier
    and in one built from the oracle's circuit caps -- and the oracle's verifier does."""
    from test_gpu_proofgen import make_ir, words
    from pg_common import ir_words
    pg = bpg.proof_gen
    cfg, log_n = chain_config(ch)
    ost = oracle.PgState(**cfg)
    b = pg.ProverStateBuilder()
    for t, name in enumerate(pg.TABLES):
        getattr(b, "set_%s_circuit_size" % name)(range(cfg["table_log_lo"][t], cfg["table_log_hi"][t]))
    b.set(**{k: v for k, v in cfg.items() if not k.startswith("table_")}, n_workers=2, arena_bytes=256 << 20)
    st = b.build()
    try:
        t0 = pg.generate_txn_proof(st, make_ir(pg, 7, 0, 0x5EED0001, log_n=log_n))
        root1 = t0.p_vals.state_root_after
        t1 = pg.generate_txn_proof(st, make_ir(pg, 7, 1, 0x5EED0002, root=root1, gas=(121, 150), log_n=log_n))
        agg = pg.generate_agg_proof(st, t0, t1)
        blk = pg.generate_block_proof(st, None, agg)
        o0 = ost.txn(ir_words(7, 0, 0x5EED0001, log_n=log_n))
        o1 = ost.txn(ir_words(7, 1, 0x5EED0002, root_before=root1, gas=(121, 150), log_n=log_n))
        oa = ost.agg(o0, False, o1, False)
        ob = ost.block(None, oa)
        for name, got, want in (("txn 0", t0, o0), ("txn 1", t1, o1), ("aggregation", agg, oa), ("block", blk, ob)):
            g = words(got.intern)
            assert g.shape == want.shape, name
            bad = np.nonzero(g != want)[0]
            assert bad.size == 0, "%s: first mismatch at word %d of %d" % (name, bad[0], want.size)
            assert ost.verify(g) == 0, name
        for v in (pg.VerifierState.from_prover_state(st), pg.VerifierState.from_caps(b.cfg, ost.circuit_caps().reshape(-1))):
            v.verify(blk)
            for p in (t0, t1, agg, blk):
                v.verify_any(p.intern)
            bad = bytearray(blk.intern)
            bad[len(bad) // 2] ^= 4
            with pytest.raises(pg.ProofGenError):
                v.verify(bytes(bad))
    finally:
        st.close()
