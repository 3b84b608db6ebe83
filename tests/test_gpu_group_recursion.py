"""A group's recursion levels as lock-step batches over the group (bp_tune_rec_group; csrc/proofgen.cpp: group_recursion,
rec_prove_batch, lockstep_cap): level k of the seven chains of all the transactions a lease holds is one batch -- 7 g
proofs on 7 g transcripts and the riders that fit, 24 at most, their argument blocks in the stream's argument ring
(csrc/arg_ring.hpp).  Every proof keeps its own circuit, public inputs and transcript, so not one byte may move: the
reference is the same shard with txn_group = 1, and rec_group = 1 (one transaction's recursion at a time) beside it.
bp_debug_rec_batch_histogram says which batch sizes were proved.
SMALL_PLONK: rec_log_n = 6, seven chains, shrink_depth = 2, 256 MiB arenas."""
import ctypes as C
import threading

import pytest

from pg_common import SMALL, SMALL_PLONK, WIDTH
from test_gpu_txn_groups import build_state, prove_shard

pytestmark = pytest.mark.gpu

BLOCK = 43
LOWEST = tuple(SMALL["table_log_lo"])
SIZES = (1, 2, 3, 5)
HIST = 32   # sizes reported: 0 .. 31 (a launch accepts 24)


@pytest.fixture(scope="module")
def pg(bpg):
    return bpg.proof_gen


@pytest.fixture(scope="module")
def L(pg):
    return pg._bind()


@pytest.fixture
def knobs(L):
    """every knob back to its default after the test"""
    try:
        yield L
    finally:
        L.bp_tune_reset()


def histogram(L, reset=True):
    out = (C.c_uint64 * HIST)()
    assert L.bp_debug_rec_batch_histogram(out, HIST, 1 if reset else 0) == 0
    return list(out)


def chain(n):
    from proof_protocol_decoder_amd.block_driver import synthetic_block_irs
    return synthetic_block_irs(BLOCK, n, LOWEST, WIDTH)


def reference_of(pg, L, cfg, sizes=SIZES):
    """txn_group = 1, rec_group = 1 on a state of two workers: the containers and the roots of the first n transactions"""
    L.bp_tune_txn_group(1)
    L.bp_tune_rec_group(1)
    st = build_state(pg, cfg, 2)
    try:
        irs = chain(max(sizes))
        roots, by_n = {}, {}
        for n in sizes:
            roots[n], by_n[n] = prove_shard(pg, st, irs[:n], 2)
        txns = by_n[max(sizes)]
        assert all(by_n[n] == txns[:n] for n in sizes)
        return irs, txns, roots
    finally:
        L.bp_tune_reset()
        st.close()


@pytest.fixture(scope="module")
def reference(pg, L):
    return reference_of(pg, L, SMALL_PLONK)


@pytest.fixture(scope="module", params=[3, 4])
def state(request, pg):
    st = build_state(pg, SMALL_PLONK, request.param)
    try:
        yield request.param, st
    finally:
        st.close()


@pytest.mark.parametrize("riders", [1, 0])
def test_group_recursion_is_the_ungrouped_bytes(pg, knobs, state, reference, riders):
    """Shards of 1, 2, 3 and 5 transactions, txn_group = 3, rec_group 0 against 1, with the riders and without: every
    container and every root is the reference's.  One thread takes the transactions three at a time, so the batch sizes are
    known: rec_group = 0 proves the 21 chain proofs of three transactions in one batch (and no batch of a size that only
    one transaction's level has, once three are held); rec_group = 1 proves none above eight."""
    n_workers, st = state
    irs, txns, roots = reference
    knobs.bp_tune_txn_group(3)
    knobs.bp_tune_rec_riders(riders)
    for rec_group in (0, 1):
        knobs.bp_tune_rec_group(rec_group)
        histogram(knobs)
        for n in SIZES:
            for n_threads in (1, n_workers):
                root, got = prove_shard(pg, st, irs[:n], n_threads)
                assert got == txns[:n], (n, rec_group, n_workers, n_threads, riders)
                assert root == roots[n], (n, rec_group, n_workers, n_threads, riders)
        h = histogram(knobs)
        print("rec_group=%d riders=%d workers=%d: batches by size %s" % (rec_group, riders, n_workers, {b: c for b, c in enumerate(h) if c}))
        if rec_group == 0:
            assert sum(h[15:]) > 0, h
            assert sum(h[25:]) == 0, h
        else:
            assert sum(h[9:]) == 0, h
            assert h[7] + h[8] > 0, h


def test_three_transactions_on_one_thread_are_two_batches_a_level(pg, knobs, state, reference):
    """The lease of one thread on three idle neighbours holds all three: shrink_depth = 2 levels of 21 proofs each, the
    three roots posted to the pool -- no batch of seven anywhere."""
    n_workers, st = state
    irs, txns, roots = reference
    knobs.bp_tune_txn_group(3)
    knobs.bp_tune_rec_group(0)
    histogram(knobs)
    root, got = prove_shard(pg, st, irs[:3], 1)
    h = histogram(knobs)
    assert got == txns[:3] and root == roots[3]
    assert h[21] + h[22] + h[23] + h[24] == SMALL_PLONK["shrink_depth"], h
    assert h[7] == 0 and h[8] == 0, h


def test_forty_queries_split_a_group_of_three_sixteen_and_five(pg, L, knobs):
    """rec_num_queries = 40: the query launches index 672 openings, so a batch holds 16 proofs and the 21 chain proofs of a
    group of three are split 16 + 5, at both levels (no rider: the chains alone pass the limit).  Nothing is refused and
    the bytes are the reference's -- on one thread, where the sizes are known, and on three."""
    cfg = dict(SMALL_PLONK, rec_num_queries=40)
    irs, txns, roots = reference_of(pg, L, cfg)
    st = build_state(pg, cfg, 3)
    try:
        knobs.bp_tune_txn_group(3)
        knobs.bp_tune_rec_group(0)
        histogram(knobs)
        root, got = prove_shard(pg, st, irs[:3], 1)
        h = histogram(knobs)
        print("rec_num_queries=40: batches by size %s" % {b: c for b, c in enumerate(h) if c})
        assert got == txns[:3] and root == roots[3]
        assert h[16] == 2 and h[5] == 2 and sum(h[17:]) == 0, h
        root, got = prove_shard(pg, st, irs, 3)
        h = histogram(knobs)
        assert got == txns and root == roots[5]
        assert sum(h[17:]) == 0, h
    finally:
        st.close()


def test_thirty_queries_leave_room_for_one_rider(pg, L, knobs):
    """rec_num_queries = 30: a batch holds 22.  Six transactions on one thread are two groups of three: the first group's
    levels are batches of 21 (nothing is ready to ride yet), and while the second group is in its levels the first
    group's roots are waiting in the pool -- each of its two levels is 21 chain proofs and ONE rider in one batch."""
    cfg = dict(SMALL_PLONK, rec_num_queries=30)
    irs, txns, roots = reference_of(pg, L, cfg, sizes=(6,))
    st = build_state(pg, cfg, 3)
    try:
        knobs.bp_tune_txn_group(3)
        knobs.bp_tune_rec_group(0)
        histogram(knobs)
        root, got = prove_shard(pg, st, irs, 1)
        h = histogram(knobs)
        print("rec_num_queries=30: batches by size %s" % {b: c for b, c in enumerate(h) if c})
        assert got == txns and root == roots[6]
        assert h[21] == 2 and h[22] == 2 and sum(h[23:]) == 0, h
    finally:
        st.close()


def test_abort_before_and_during_the_recursion(pg, knobs, state, reference):
    """A flag raised before the call, and one raised from another thread once the first recursion batch has started (the
    histogram says so): BP_ERR_ABORTED both times, and the next call on the same state -- every worker, rider and job of
    the aborted one given back -- proves the reference's bytes."""
    n_workers, st = state
    irs, txns, roots = reference
    knobs.bp_tune_txn_group(3)
    knobs.bp_tune_rec_group(0)
    flag = C.c_uint8(1)
    with pytest.raises(pg.ProofGenError) as e:
        prove_shard(pg, st, irs, n_workers, abort=flag)
    assert e.value.code == -1
    flag.value = 0
    root, got = prove_shard(pg, st, irs[:3], 1, abort=flag)
    assert got == txns[:3] and root == roots[3]

    histogram(knobs)
    done = threading.Event()

    def raise_in_the_recursion():
        while not done.is_set():
            if sum(histogram(knobs, reset=False)):
                flag.value = 1
                return

    t = threading.Thread(target=raise_in_the_recursion)
    t.start()
    try:
        with pytest.raises(pg.ProofGenError) as e:
            prove_shard(pg, st, irs, 1, abort=flag)
    finally:
        done.set()
        t.join()
    assert e.value.code == -1
    assert flag.value == 1, "the shard ended before its first recursion batch started"
    flag.value = 0
    root, got = prove_shard(pg, st, irs, n_workers, abort=flag)
    assert got == txns and root == roots[5]


def test_a_lone_transaction_with_side_lanes(pg, bpg, knobs, reference):
    """One transaction on a state of four workers, side lanes on: its trace commitments are queued on the streams of
    borrowed workers and read their argument blocks from those workers' rings.  The bytes are the reference's, with the
    lanes off as well."""
    irs, txns, roots = reference
    st = build_state(pg, SMALL_PLONK, 4)
    try:
        with bpg.ops.tuned(side_lanes=1):
            assert bytes(pg.generate_txn_proof(st, irs[0]).intern) == txns[0]
            root, got = prove_shard(pg, st, irs[:1], 1)
            assert got == txns[:1] and root == roots[1]
        with bpg.ops.tuned(side_lanes=0):
            assert bytes(pg.generate_txn_proof(st, irs[0]).intern) == txns[0]
    finally:
        st.close()
