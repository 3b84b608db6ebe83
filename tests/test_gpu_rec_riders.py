"""Root and aggregation proofs as riders (csrc/rec_pool.hpp, bp_tune_rec_riders): inside bp_prove_shard and
bp_aggregate_proofs they are proved in the spare slot of other transactions' lock-step batches, or a batch at a time at
the end of the tree.  Every proof has its own transcript, so not one byte may move: the reference here is the inline
path -- bp_generate_txn_proof per IR, then bp_generate_agg_proof along aggregation_plan(n, shape) -- never the code
under test."""
import ctypes as C

import numpy as np
import pytest

from pg_common import LOG_N, SMALL, SMALL_PLONK, WIDTH
from proof_protocol_decoder_amd._abi import ShardOptions as Opt

pytestmark = pytest.mark.gpu

BLOCK = 41
N_MAX = 9          # the reference chain: the shards take its first 1, 2 and 5 transactions, bp_aggregate_proofs 5 and 9
SHAPES = ("balanced", "pairs_then_chain")


def words(b):
    return np.frombuffer(b, dtype=np.uint64)


def build_state(pg, cfg, n_workers=3):
    b = pg.ProverStateBuilder()
    for t, name in enumerate(pg.TABLES):
        getattr(b, "set_%s_circuit_size" % name)(range(cfg["table_log_lo"][t], cfg["table_log_hi"][t]))
    b.set(**{k: v for k, v in cfg.items() if not k.startswith("table_")}, n_workers=n_workers, arena_bytes=256 << 20)
    return b.build()


def prove_shard(pg, st, irs, n_threads, shape, abort=None):
    """bp_prove_shard itself: (root bytes, [txn proof bytes])"""
    from proof_protocol_decoder_amd.block_driver import TREE_SHAPES
    L = pg._bind()
    u8p = C.POINTER(C.c_uint8)
    n = len(irs)
    raw = b"".join(ir.to_bytes() for ir in irs)
    root, root_len = u8p(), C.c_size_t()
    leaves, lens = (u8p * n)(), (C.c_size_t * n)()
    opt = Opt(n_threads, TREE_SHAPES[shape])
    pg.check(L.bp_prove_shard(st._h, raw, len(raw) // n, n, C.byref(opt), C.byref(abort) if abort is not None else None,
                              C.byref(root), C.byref(root_len), leaves, lens))
    return pg.take_buffer(root, root_len), [pg.take_buffer(leaves[i], C.c_size_t(lens[i])) for i in range(n)]


def aggregate_proofs(pg, st, raws, n_threads, shape):
    from proof_protocol_decoder_amd.block_driver import TREE_SHAPES
    L = pg._bind()
    n = len(raws)
    ptrs = (C.c_char_p * n)(*raws)
    lens = (C.c_size_t * n)(*[len(r) for r in raws])
    out, out_len = C.POINTER(C.c_uint8)(), C.c_size_t()
    opt = Opt(n_threads, TREE_SHAPES[shape])
    pg.check(L.bp_aggregate_proofs(st._h, ptrs, lens, n, C.byref(opt), C.byref(out), C.byref(out_len)))
    return pg.take_buffer(out, out_len)


class Reference:
    """The inline path, once per state: the txn proofs of the chain, and on demand the tree over the first n of them."""

    def __init__(self, pg, st, n):
        from proof_protocol_decoder_amd.block_driver import synthetic_block_irs
        self.pg, self.st = pg, st
        self.irs = synthetic_block_irs(BLOCK, n, LOG_N, WIDTH)
        self.txns = [pg.generate_txn_proof(st, ir) for ir in self.irs]
        self._roots = {}

    def root(self, n, shape):
        from proof_protocol_decoder_amd.block_driver import aggregation_plan
        if (n, shape) not in self._roots:
            nodes = list(self.txns[:n])
            for l, r in aggregation_plan(n, shape):
                nodes.append(self.pg.generate_agg_proof(self.st, nodes[l], nodes[r]))
            self._roots[(n, shape)] = bytes(nodes[-1].intern)
        return self._roots[(n, shape)]

    def txn_bytes(self, n):
        return [bytes(t.intern) for t in self.txns[:n]]


@pytest.fixture(scope="module")
def pg(bpg):
    return bpg.proof_gen


@pytest.fixture(scope="module", params=["synthetic", "plonk"])
def kit(request, pg):
    """(cfg, state, reference) for the small state with the synthetic and with the PLONK-shaped recursion circuit"""
    cfg = SMALL if request.param == "synthetic" else SMALL_PLONK
    st = build_state(pg, cfg)
    try:
        yield cfg, st, Reference(pg, st, N_MAX)
    finally:
        st.close()


@pytest.fixture
def riders_off(pg):
    L = pg._bind()
    L.bp_tune_rec_riders(0)
    try:
        yield
    finally:
        L.bp_tune_reset()


@pytest.mark.parametrize("n_threads", [1, 2, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_shard_of_five_is_the_inline_path_byte_for_byte(pg, oracle, kit, n_threads, shape):
    """n = 5 is odd (a carried tail); with one thread every root rides in the next transaction's first batch, with three
    the riders and the drained batches mix.  Both verifiers accept the root."""
    cfg, st, ref = kit
    root, txns = prove_shard(pg, st, ref.irs[:5], n_threads, shape)
    assert txns == ref.txn_bytes(5)
    assert root == ref.root(5, shape)
    pg.VerifierState.from_prover_state(st).verify_any(root)
    assert oracle.PgState(**cfg).verify(words(root)) == 0


@pytest.mark.parametrize("n", [1, 2])
def test_drain_only_paths(pg, kit, n):
    """One thread.  n = 1: the root IS the leaf and nobody is left to carry it.  n = 2: the only aggregation becomes
    ready after the last leaf."""
    _, st, ref = kit
    for shape in SHAPES:
        root, txns = prove_shard(pg, st, ref.irs[:n], 1, shape)
        assert txns == ref.txn_bytes(n)
        assert root == (ref.txn_bytes(1)[0] if n == 1 else ref.root(2, shape))


@pytest.mark.parametrize("n", [5, 9])
def test_aggregate_proofs_in_batches(pg, kit, n):
    """bp_aggregate_proofs has no transaction to ride with: its aggregations are proved a batch at a time (nine children:
    four of the first level at once, more than one batch in all)."""
    _, st, ref = kit
    for n_threads in (1, 3):
        assert aggregate_proofs(pg, st, ref.txn_bytes(n), n_threads, "balanced") == ref.root(n, "balanced")
    assert aggregate_proofs(pg, st, ref.txn_bytes(n), 2, "pairs_then_chain") == ref.root(n, "pairs_then_chain")


def test_riders_off_gives_the_same_bytes(pg, kit, riders_off):
    _, st, ref = kit
    for n_threads, shape in ((1, "balanced"), (3, "pairs_then_chain")):
        root, txns = prove_shard(pg, st, ref.irs[:5], n_threads, shape)
        assert txns == ref.txn_bytes(5) and root == ref.root(5, shape)
    root, txns = prove_shard(pg, st, ref.irs[:1], 1, "balanced")
    assert root == txns[0] == ref.txn_bytes(1)[0]
    assert aggregate_proofs(pg, st, ref.txn_bytes(9), 3, "balanced") == ref.root(9, "balanced")


def test_a_failing_leaf_is_the_calls_status_and_leaves_nothing_behind(pg, kit):
    """One IR of the five asks for a Keccak table outside the state's range: BP_ERR_RANGE, the message names the table;
    the same state then proves the good shard (no worker, rider or job of the failed call is left)."""
    import dataclasses
    _, st, ref = kit
    log_n = list(LOG_N)
    log_n[3] = SMALL["table_log_hi"][3]
    for n_threads in (1, 3):
        bad = list(ref.irs[:5])
        bad[3] = dataclasses.replace(bad[3], table_log_n=tuple(log_n))
        with pytest.raises(pg.ProofGenError) as e:
            prove_shard(pg, st, bad, n_threads, "balanced")
        assert e.value.code == -3 and "keccak" in e.value.message
        root, txns = prove_shard(pg, st, ref.irs[:5], n_threads, "balanced")
        assert txns == ref.txn_bytes(5) and root == ref.root(5, "balanced")


def test_abort_flag_set_before_the_call(pg, kit):
    _, st, ref = kit
    flag = C.c_uint8(1)
    for n_threads in (1, 3):
        with pytest.raises(pg.ProofGenError) as e:
            prove_shard(pg, st, ref.irs[:5], n_threads, "balanced", abort=flag)
        assert e.value.code == -1
    flag.value = 0
    root, _ = prove_shard(pg, st, ref.irs[:2], 2, "balanced", abort=flag)
    assert root == ref.root(2, "balanced")


def test_a_state_whose_batches_hold_seven_carries_no_rider(pg):
    """rec_num_queries = 33: 256 query indices per launch / 33 = 7 proofs per batch, the seven chains fill it.  Roots and
    aggregations are then proved in batches of their own, and the bytes are still the inline path's."""
    cfg = dict(SMALL_PLONK, rec_num_queries=33)
    st = build_state(pg, cfg)
    try:
        ref = Reference(pg, st, 3)
        for n_threads in (1, 3):
            root, txns = prove_shard(pg, st, ref.irs, n_threads, "balanced")
            assert txns == ref.txn_bytes(3) and root == ref.root(3, "balanced")
    finally:
        st.close()
