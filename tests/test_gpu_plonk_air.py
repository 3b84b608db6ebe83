"""AIR 8 (plonk, csrc/air.hpp: gates + the copy-constraint permutation argument) on the GPU against the oracle's
independent statement (oracle/plonk_air.c): the preprocessed constants and the witness of the fixed circuit, K5 alone
through bp_quotient_eval(air_id = 8, ...), and whole proofs byte for byte -- at 2^13 rows with 28 queries this is the
shape of upstream's recursion proofs (CircuitConfig::standard_recursion_config)."""
import ctypes as C

import numpy as np
import pytest

from builtin_airs import product_verify
from proof_protocol_decoder_amd._abi import PlonkLayout as Layout
from util import P, coset_major_to_natural, rand_field, to_dev, to_host

pytestmark = pytest.mark.gpu
SEED, CSEED = 0x5EED000000000008, 0xC0DE000000000008


def dev_constants(bpg, log_n, seed, pi_len=4, n_paths=0, depth=0, path_pi0=0, leaf_len=0):
    import torch
    out = torch.empty((85, 1 << log_n), dtype=torch.int64, device="cuda")
    L = bpg.lib()
    lay = Layout(pi_len, n_paths, depth, path_pi0, leaf_len)
    bpg._lib.check(L.bp_plonk_constants(C.c_uint64(seed), log_n, C.byref(lay), C.c_void_p(out.data_ptr()), None))
    return out


# (log_n, pi_len, n_paths, depth, path_pi0): lists of every chunking; the aggregation / block / root / chain layouts at default depth 12
CIRCUITS = [(5, 4, 0, 0, 0, 0), (8, 6, 0, 0, 0, 0), (13, 41, 0, 0, 0, 0), (6, 23, 0, 0, 0, 0), (5, 64, 0, 0, 0, 0), (5, 8, 0, 0, 0, 0),
            (5, 1, 0, 0, 0, 0), (5, 104, 0, 0, 0, 0), (13, 39, 2, 12, 10, 0), (13, 30, 1, 12, 9, 0), (13, 97, 7, 12, 28, 0),
            (13, 14, 1, 14, 6, 0), (13, 14, 1, 27, 6, 0), (6, 39, 2, 5, 10, 0), (7, 64, 2, 32, 40, 0), (7, 104, 3, 32, 80, 0),
            (5, 17, 1, 1, 3, 0),
            # the aggregation / block circuits of the default shape: they hash the 135-word rows their paths start from
            (13, 39, 2, 12, 10, 135), (13, 30, 1, 12, 9, 135), (7, 39, 2, 5, 10, 19), (7, 30, 1, 7, 9, 135),
            (13, 97, 7, 12, 28, 135), (13, 14, 1, 12, 6, 135), (6, 14, 1, 5, 6, 135)]   # ... the root and shrink circuits too


@pytest.mark.parametrize("log_n,pi_len,n_paths,depth,path_pi0,leaf_len", CIRCUITS)
def test_constants_and_witness_match_oracle(bpg, oracle, log_n, pi_len, n_paths, depth, path_pi0, leaf_len):
    """The circuit of a pi_len-word public-input list that walks n_paths Merkle paths (selectors, Poseidon-row selector,
    sigmas with the sponge's and the paths' copy cycles) and its witness (the Poseidon rows made on the host, the rest on
    the device) against the oracle's."""
    import torch
    from test_plonk_air import merkle_fixture
    k = dev_constants(bpg, log_n, CSEED + log_n, pi_len, n_paths, depth, path_pi0, leaf_len)
    want_k = oracle.plonk_constants(log_n, CSEED + log_n, pi_len, n_paths, depth, path_pi0, leaf_len)
    assert (to_host(k) == want_k).all()
    pub, lst = oracle.stark_public_inputs(SEED + log_n), oracle.stark_public_input_list(SEED + log_n)
    got_pub, got_lst = (C.c_uint64 * 4)(), (C.c_uint64 * 4)()
    bpg.lib().bp_stark_public_inputs(C.c_uint64(SEED + log_n), got_pub)
    bpg.lib().bp_stark_public_input_list(C.c_uint64(SEED + log_n), got_lst)
    assert [int(x) for x in got_pub] == [int(x) for x in pub] and [int(x) for x in got_lst] == [int(x) for x in lst]
    assert [int(x) for x in oracle.hash_no_pad(lst)] == [int(x) for x in pub]
    rng = np.random.default_rng(pi_len)
    pi = rng.integers(0, 0xFFFFFFFF00000001, size=pi_len, dtype=np.uint64)
    words, wit = merkle_fixture(oracle, rng, min(depth, 8), n_paths, cap_height=0, leaf_len=leaf_len) if depth <= 8 else (None, None)
    if n_paths and words is None:   # deep paths: any siblings will do for witness parity (the path's end is whatever it is)
        words = [int(x) for x in rng.integers(0, 0xFFFFFFFF00000001, size=8 * n_paths, dtype=np.uint64)]
        wit = []
        for _ in range(n_paths):
            wit += [int(rng.integers(0, 1 << depth))] + [int(x) for x in rng.integers(0, 0xFFFFFFFF00000001, size=4 * depth + leaf_len, dtype=np.uint64)]
    if n_paths:
        pi[path_pi0:path_pi0 + 8 * n_paths] = words
    t = torch.empty((135, 1 << log_n), dtype=torch.int64, device="cuda")
    pi_c = (C.c_uint64 * pi_len)(*[int(x) for x in pi])
    wit_c = (C.c_uint64 * max(1, len(wit or [])))(*[int(x) for x in (wit or [])])
    lay = Layout(pi_len, n_paths, depth, path_pi0, leaf_len)
    bpg._lib.check(bpg.lib().bp_plonk_trace(C.c_void_p(k.data_ptr()), C.c_uint64(SEED + log_n), pi_c, C.byref(lay), wit_c if n_paths else None,
                                            log_n, C.c_void_p(t.data_ptr()), None))
    got = to_host(t)
    assert (got == oracle.plonk_trace(log_n, SEED + log_n, pi, want_k, n_paths, depth, path_pi0, wit, leaf_len)).all()
    assert [int(x) for x in got[:4, 0]] == [int(x) for x in oracle.hash_no_pad(pi)]


def test_layouts_that_do_not_fit_are_refused(bpg):
    from proof_protocol_decoder_amd._lib import BpgError
    for log_n, lay in ((5, (39, 2, 12, 10)), (13, (39, 2, 12, 32)), (13, (105, 0, 0, 0)), (13, (39, 4, 30, 0)), (13, (0, 0, 0, 0)), (4, (4, 0, 0, 0)),
                       (13, (39, 2, 12, 10, 8)), (13, (39, 0, 0, 0, 135)), (13, (39, 2, 12, 10, 500)), (6, (39, 2, 5, 10, 135))):
        with pytest.raises(BpgError):
            dev_constants(bpg, log_n, 1, *lay)


@pytest.mark.parametrize("log_n,loaded", [(5, 0), (9, 1), (13, 0)])
def test_quotient_eval_matches_oracle(bpg, oracle, log_n, loaded):
    """K5 alone on AIR 8: random LDE matrices (gates, and the chunk relations of the copy products with the row's point
    x and the sigmas from the constants matrix), fixed challenges, public inputs zero."""
    rng = np.random.default_rng(800 + log_n)
    rows = (1 << log_n) << 3
    trace, aux, consts = rand_field(rng, (135, rows)), rand_field(rng, (20, rows)), rand_field(rng, (85, rows))
    ctl, alphas = rand_field(rng, (4,)), rand_field(rng, (2,))
    want = oracle.quotient_values(oracle.plonk_cfg(log_n), consts, trace, aux, ctl, alphas[0], alphas[1])
    idx = coset_major_to_natural(log_n, 3)

    def to_cm(mat):
        cm = np.empty_like(mat)
        cm[:, idx] = mat
        return to_dev(cm)
    with bpg.ops.tuned(assume_loaded=loaded):
        got = bpg.ops.quotient_eval(bpg.ops.stark_cfg(log_n, 135, n_const=85, deg_pow=3, rate_bits=3), to_cm(trace), to_cm(aux),
                                    to_cm(consts), ctl, alphas, air_id=8)
    assert (to_host(got)[:, idx] == want).all()


def oracle_proof(oracle, log_n, nq, pb, seed, cseed):
    pub = oracle.stark_public_inputs(seed)
    cfg = oracle.plonk_cfg(log_n, pub=pub, num_queries=nq, pow_bits=pb)
    k = oracle.plonk_constants(log_n, cseed)
    tr = oracle.plonk_trace(log_n, seed, oracle.stark_public_input_list(seed), k)
    cc = oracle.Committed.from_values(k, 3, 4)
    tc = oracle.Committed.from_values(tr, 3, 4)
    ch = oracle.PyChallenger()
    ch.observe(cc.cap())
    ch.observe(tc.cap())
    ctl = np.array([ch.challenge() for _ in range(4)], dtype=np.uint64)
    chv = ch.clone()
    return cfg, oracle.stark_prove(cfg, tr, ctl, ch, cc, tc), ctl, chv, cc.cap().copy(), pub


@pytest.mark.parametrize("log_n,nq,pb,loaded", [(5, 6, 6, 0), (9, 20, 10, 1), (13, 28, 16, 0), (13, 28, 16, 1)])
def test_proof_bit_exact(bpg, oracle, log_n, nq, pb, loaded):
    cfg, want, ctl, chv, cap, pub = oracle_proof(oracle, log_n, nq, pb, SEED, CSEED)
    pc = bpg.ops.stark_cfg(log_n, 135, n_const=85, deg_pow=3, rate_bits=3, num_queries=nq, pow_bits=pb)
    with bpg.ops.tuned(assume_loaded=loaded):
        got = bpg.ops.stark_prove_air(8, pc, SEED, const_seed=CSEED)
    assert got.shape == want.shape and int(got[14]) == 8 and int(got[4]) == 20
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "first mismatch at word %d of %d" % (bad[0], want.size)
    assert oracle.stark_verify(cfg, got, ctl, chv, cap) == 0
    assert product_verify(pc, 8, got, cap, pub) == 0
    flipped = got.copy()
    flipped[got.size // 2] ^= np.uint64(1 << 21)
    assert product_verify(pc, 8, flipped, cap, pub) != 0
    wrong = [int(x) for x in pub]
    wrong[0] ^= 2
    assert product_verify(pc, 8, got, cap, wrong) != 0


def test_wrong_shapes_for_the_air_are_refused(bpg):
    from proof_protocol_decoder_amd._lib import BpgError
    for kw in (dict(n_cols=136, n_const=85, deg_pow=3, rate_bits=3), dict(n_cols=135, n_const=84, deg_pow=3, rate_bits=3),
               dict(n_cols=135, n_const=85)):
        cfg = bpg.ops.stark_cfg(6, kw.pop("n_cols"), num_queries=6, pow_bits=6, **kw)
        with pytest.raises(BpgError, match="plonk"):
            bpg.ops.stark_prove_air(8, cfg, 1)


def test_recursion_layer_on_the_plonk_circuit_matches_the_oracle(bpg, oracle):
    """bp_config.rec_air_id = 8: the seven per-table chains (in lock-step batches), the root proof, an aggregation and a
    block proof are proofs of the PLONK-shaped circuit; containers equal the oracle's byte for byte, both verifiers
    accept, lock-step batching does not change a byte."""
    import struct
    from pg_common import LOG_N, SMALL_PLONK, WIDTH, ir_words
    pg = bpg.proof_gen
    b = pg.ProverStateBuilder()
    for t, name in enumerate(pg.TABLES):
        getattr(b, "set_%s_circuit_size" % name)(range(SMALL_PLONK["table_log_lo"][t], SMALL_PLONK["table_log_hi"][t]))
    b.set(**{k: v for k, v in SMALL_PLONK.items() if not k.startswith("table_")}, n_workers=2, arena_bytes=256 << 20)
    st, ost = b.build(), oracle.PgState(**SMALL_PLONK)
    try:
        ir0 = pg.TxnProofGenIR(7, 0, 100, 121, (1, 2, 3, 4), 0x5EED0001, tuple(LOG_N), tuple(WIDTH))
        t0 = pg.generate_txn_proof(st, ir0)
        o0 = ost.txn(ir_words(7, 0, 0x5EED0001))
        got = np.frombuffer(t0.intern, dtype=np.uint64)
        assert got.shape == o0.shape and (got == o0).all()
        t1 = pg.generate_txn_proof(st, pg.TxnProofGenIR(7, 1, 121, 150, t0.p_vals.state_root_after, 0x5EED0002, tuple(LOG_N), tuple(WIDTH)))
        o1 = ost.txn(ir_words(7, 1, 0x5EED0002, root_before=t0.p_vals.state_root_after, gas=(121, 150)))
        agg = pg.generate_agg_proof(st, t0, t1)
        oa = ost.agg(o0, False, o1, False)
        assert (np.frombuffer(agg.intern, dtype=np.uint64) == oa).all()
        blk = pg.generate_block_proof(st, None, agg)
        assert (np.frombuffer(blk.intern, dtype=np.uint64) == ost.block(None, oa)).all()
        pg.VerifierState.from_prover_state(st).verify(blk)
        assert ost.verify(np.frombuffer(blk.intern, dtype=np.uint64)) == 0
        with bpg.ops.tuned(rec_batch=1):
            assert pg.generate_txn_proof(st, ir0).intern == t0.intern
    finally:
        st.close()
