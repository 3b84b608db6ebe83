"""Several transactions at a time (bp_tune_txn_group; csrc/proofgen.cpp: ProverLease, prove_tables -- the one path of
every transaction, a lone one being a group of one; csrc/rec_pool.hpp: the scheduler's group rule): a thread of bp_prove_shard / bp_prove_shard_gi leases a run of neighbouring provers and proves
table t of its transactions in lock-step wherever their shapes agree.  Every transaction keeps its own transcript, so not
one byte may move: the reference is the same call with txn_group = 1 (and, once, the inline path and the oracle's
verifier, as tests/test_gpu_rec_riders.py has them), the table-proof blobs of the single call for the group call.
Small states: the smallest heights of every range, 256 MiB arenas."""
import ctypes as C
import dataclasses
import struct

import numpy as np
import pytest

import txn_table_cases as tc
from pg_common import SMALL, SMALL_PLONK, WIDTH
from proof_protocol_decoder_amd._abi import ShardOptions as Opt

pytestmark = pytest.mark.gpu

BLOCK = 43
LOWEST = tuple(SMALL["table_log_lo"])   # (6, 5, 6, 7, 5, 6, 8)
SIZES = (1, 2, 3, 5)                    # a lone transaction, a whole group, a remainder, two groups and a remainder


def words(b):
    return np.frombuffer(b, dtype=np.uint64)


def build_state(pg, cfg, n_workers):
    b = pg.ProverStateBuilder()
    for t, name in enumerate(pg.TABLES):
        getattr(b, "set_%s_circuit_size" % name)(range(cfg["table_log_lo"][t], cfg["table_log_hi"][t]))
    b.set(**{k: v for k, v in cfg.items() if not k.startswith("table_")}, n_workers=n_workers, arena_bytes=256 << 20)
    return b.build()


def prove_shard(pg, st, irs, n_threads, abort=None):
    """bp_prove_shard itself: (root bytes, [txn proof bytes])"""
    L = pg._bind()
    u8p = C.POINTER(C.c_uint8)
    n = len(irs)
    raw = b"".join(ir.to_bytes() for ir in irs)
    root, root_len = u8p(), C.c_size_t()
    leaves, lens = (u8p * n)(), (C.c_size_t * n)()
    opt = Opt(n_threads, 0)
    pg.check(L.bp_prove_shard(st._h, raw, len(raw) // n, n, C.byref(opt), C.byref(abort) if abort is not None else None,
                              C.byref(root), C.byref(root_len), leaves, lens))
    return pg.take_buffer(root, root_len), [pg.take_buffer(leaves[i], C.c_size_t(lens[i])) for i in range(n)]


@pytest.fixture(scope="module")
def pg(bpg):
    return bpg.proof_gen


@pytest.fixture
def group(pg):
    """sets bp_tune_txn_group for the test, and puts every knob back after it"""
    L = pg._bind()
    try:
        yield lambda g: L.bp_tune_txn_group(g)
    finally:
        L.bp_tune_reset()


def chain(n, log_n=LOWEST):
    from proof_protocol_decoder_amd.block_driver import synthetic_block_irs
    return synthetic_block_irs(BLOCK, n, log_n, WIDTH)


@pytest.fixture(scope="module")
def reference(pg):
    """txn_group = 1 on a state of its own, once: the five transactions' containers and the roots of the first n of them"""
    L = pg._bind()
    L.bp_tune_txn_group(1)
    st = build_state(pg, SMALL_PLONK, 2)
    try:
        irs = chain(max(SIZES))
        roots, by_n = {}, {}
        for n in SIZES:
            roots[n], by_n[n] = prove_shard(pg, st, irs[:n], 2)
        txns = by_n[max(SIZES)]
        assert all(by_n[n] == txns[:n] for n in SIZES)
        yield irs, txns, roots
    finally:
        L.bp_tune_reset()
        st.close()


@pytest.fixture(scope="module", params=[2, 3, 4])
def state(request, pg):
    st = build_state(pg, SMALL_PLONK, request.param)
    try:
        yield request.param, st
    finally:
        st.close()


@pytest.mark.parametrize("g", [1, 2, 3])
def test_shards_are_the_ungrouped_bytes(pg, state, reference, group, g):
    """n in {1, 2, 3, 5} x txn_group x n_workers: remainders, a group larger than the shard, worker counts that are no
    multiple of the group."""
    n_workers, st = state
    irs, txns, roots = reference
    group(g)
    for n in SIZES:
        root, got = prove_shard(pg, st, irs[:n], n_workers)
        assert got == txns[:n], (n, g, n_workers)
        assert root == roots[n], (n, g, n_workers)


def test_more_threads_than_workers_and_the_inline_path(pg, oracle, state, reference, group):
    """Six threads on two to four workers; the root is also the inline path's (bp_generate_txn_proof per IR, then
    bp_generate_agg_proof along the plan) and both verifiers accept it."""
    from proof_protocol_decoder_amd.block_driver import aggregation_plan
    n_workers, st = state
    irs, txns, roots = reference
    group(2)
    root, got = prove_shard(pg, st, irs, 6)
    assert got == txns and root == roots[5]
    if n_workers == 3:
        nodes = [pg.generate_txn_proof(st, ir) for ir in irs]
        assert [bytes(t.intern) for t in nodes] == txns
        for l, r in aggregation_plan(5, "balanced"):
            nodes.append(pg.generate_agg_proof(st, nodes[l], nodes[r]))
        assert bytes(nodes[-1].intern) == root
        pg.VerifierState.from_prover_state(st).verify_any(root)
        assert oracle.PgState(**SMALL_PLONK).verify(words(root)) == 0


def test_mixed_shapes_in_one_group(pg, state, group):
    """The second transaction of three differs in the height of two tables, the widest (keccak) among them: tables 3 and 6
    are sub-batches of two and one, the other five sub-batches of three (of two on two workers)."""
    n_workers, st = state
    irs = chain(3)
    log_n = list(LOWEST)
    log_n[3] += 1
    log_n[6] += 1
    irs[1] = dataclasses.replace(irs[1], table_log_n=tuple(log_n))
    group(1)
    want = prove_shard(pg, st, irs, 1)
    for g in (2, 3):
        group(g)
        assert prove_shard(pg, st, irs, n_workers) == want, g


# ---- every built-in AIR in a batch: the table-proof blobs of the group call against the single call's ----
def case_words(case, k):
    w = tc.ir_words(case)
    w[10] = tc.SEED + 0x101 * k   # another seed, another witness: the proofs of a batch differ
    return w


def with_heights(case, log_n):
    return case._replace(log_n=tuple(log_n))


def group_call(pg, st, cases_words):
    """(status, message, [blobs]) of bp_generate_txn_table_proofs_group over (case, words) pairs"""
    L = pg._bind()
    n = len(cases_words)
    structs = [tc.witness_struct(pg, c) for c, _ in cases_words]
    data = (C.c_void_p * n)(*[C.addressof(w) if w is not None else None for w, _ in structs])
    outs, lens = (C.POINTER(C.c_uint8) * n)(), (C.c_size_t * n)()
    raw = b"".join(struct.pack("<25Q", *w) for _, w in cases_words)
    rc = L.bp_generate_txn_table_proofs_group(st._h, raw, 200, n, data, None, outs, lens)
    del structs
    if rc:
        assert all(not outs[i] for i in range(n)), "a failed call handed out a blob"
        return rc, L.bp_last_error().decode(), None
    return 0, "", [pg.take_buffer(outs[i], C.c_size_t(lens[i])) for i in range(n)]


@pytest.fixture(scope="module")
def air_state(pg):
    b = pg.ProverStateBuilder()
    for t, name in enumerate(pg.TABLES):
        getattr(b, "set_%s_circuit_size" % name)(range(tc.CFG["table_log_lo"][t], tc.CFG["table_log_hi"][t]))
    b.set(**{k: v for k, v in tc.CFG.items() if not k.startswith("table_")}, n_workers=3, arena_bytes=256 << 20)
    st = b.build()
    try:
        yield st
    finally:
        st.close()


BY_NAME = {c.name: c for c in tc.CASES}
# AIRs 1 .. 6 together, and AIR 7 with the other five, seeded, at the lowest heights of the ranges; then caller-given data
AIR_CASES = [with_heights(BY_NAME["six_together"], LOWEST), with_heights(BY_NAME["mul_with_the_other_five"], LOWEST),
             BY_NAME["keccak_full"], BY_NAME["logic_fits_behind_the_xors"], BY_NAME["arithmetic_given_under_mul"]]


@pytest.mark.parametrize("case", AIR_CASES, ids=[c.name for c in AIR_CASES])
def test_every_air_in_batches_of_two_and_three(pg, bpg, air_state, case):
    """... and in a batch of ONE, which is the single call: once with side_lanes at its default (the lone prover borrows the
    streams of air_state's two idle workers for its trace commitments), once with the borrowing switched off."""
    singles = []
    for k in range(3):
        rc, msg, blob = tc.table_proofs(pg, air_state, case, case_words(case, k))
        assert rc == 0, msg
        singles.append(blob)
    assert len(set(singles)) == 3
    for b in (1, 2, 3):
        rc, msg, blobs = group_call(pg, air_state, [(case, case_words(case, k)) for k in range(b)])
        assert rc == 0, msg
        assert blobs == singles[:b], (case.name, b)
    with bpg.ops.tuned(side_lanes=0):
        rc, msg, blobs = group_call(pg, air_state, [(case, case_words(case, 0))])
    assert rc == 0, msg
    assert blobs == singles[:1], case.name


def test_side_lanes_belong_to_a_lone_transaction(pg, bpg, reference, group):
    """side_lanes = 3 on four workers: a group of two counts as two provers and would pass the knob's test, but lanes are
    for a group of ONE -- the two transactions are committed in lock-step and give the reference's bytes.  So do the same
    two, one after the other on one thread, with the lanes switched off."""
    irs, txns, roots = reference
    st = build_state(pg, SMALL_PLONK, 4)
    try:
        with bpg.ops.tuned(side_lanes=3):
            group(2)
            root, got = prove_shard(pg, st, irs[:2], 1)
        assert got == txns[:2] and root == roots[2]
        with bpg.ops.tuned(side_lanes=0):
            group(1)
            root, got = prove_shard(pg, st, irs[:2], 1)
        assert got == txns[:2] and root == roots[2]
    finally:
        st.close()


def test_a_decoded_entry_with_its_own_witness_beside_seeded_ones(pg, air_state):
    """Four tables of the decoded entry hold the caller's data (Keccak-f, sponge, memory, byte packing); it is grouped
    with a copy of itself and with a seeded transaction of other heights."""
    case, w = tc.decoded_case()
    seeded = with_heights(BY_NAME["six_together"], LOWEST)
    members = [(case, w), (seeded, case_words(seeded, 1)), (case, w)]
    singles = []
    for c, cw in members[:2]:
        rc, msg, blob = tc.table_proofs(pg, air_state, c, cw)
        assert rc == 0, msg
        singles.append(blob)
    rc, msg, blobs = group_call(pg, air_state, members)
    assert rc == 0, msg
    assert blobs == [singles[0], singles[1], singles[0]]


def test_decoded_block_through_prove_shard_gi(pg, air_state, group):
    """bp_prove_shard_gi: the entries' IRs and witnesses are made in the library, the entries differ in their heights"""
    import test_decoding as td
    from proof_protocol_decoder_amd import decoding
    from proof_protocol_decoder_amd.block_driver import BlockDriver, GiOptions
    from pg_common import LOG_N
    m = td.fresh_model()
    infos = [t for t, _ in td.block(m)]
    other = decoding.OtherBlockData(decoding.BlockLevelData(b"meta", b"hashes", [(td.B, 100)]), b"\x22" * 32)
    geni = decoding.generation_inputs_bytes(td.make_trace(m, infos, hash_out_storage_of=(td.E,)), other)
    opts = GiOptions.make(24, LOG_N, WIDTH, keccak_air=True, keccak_trie_nodes=True, memory_air=True, byte_packing_air=True,
                          keccak_sponge_air=True)
    n = min(3, len(pg_gi_count(pg, geni)))
    drv = BlockDriver(air_state, n_threads=3)
    try:
        group(1)
        top, leaves = drv.prove_shard_gi(geni, 0, n, opts)
        for g in (2, 3):
            group(g)
            top_g, leaves_g = drv.prove_shard_gi(geni, 0, n, opts)
            assert [p.intern for p in leaves_g] == [p.intern for p in leaves] and top_g.intern == top.intern, g
    finally:
        drv.close()


def pg_gi_count(pg, geni):
    L = pg._bind()
    n = C.c_uint32()
    pg.check(L.bp_gi_count(geni, len(geni), C.byref(n)))
    return range(n.value)


# ---- failures ----
def test_a_bad_witness_in_a_group_fails_as_it_does_alone(pg, air_state):
    """The decoded entry's memory log with one read that returns something else than was written, grouped behind a good
    transaction: the status and the message of the single call, no blob, and the state goes on proving."""
    case, w = tc.decoded_case()
    bad_log = [list(r) for r in case.witness[6]]
    k = next(i for i, r in enumerate(bad_log) if r[0] == 1)
    bad_log[k][3] ^= 1
    bad = case._replace(witness={**case.witness, 6: bad_log})
    rc1, msg1, _ = tc.table_proofs(pg, air_state, bad, w)
    assert rc1 == -5 and "memory does not satisfy its AIR" in msg1
    rc, msg, _ = group_call(pg, air_state, [(case, w), (bad, w)])
    assert (rc, msg) == (rc1, msg1)
    rc, msg, blobs = group_call(pg, air_state, [(case, w), (case, w)])
    assert rc == 0 and blobs[0] == blobs[1] == tc.table_proofs(pg, air_state, case, w)[2]


def test_a_height_out_of_range_in_a_group_fails_as_it_does_alone(pg, state, reference, group):
    n_workers, st = state
    irs, txns, roots = reference
    log_n = list(LOWEST)
    log_n[3] = SMALL["table_log_hi"][3]
    bad = list(irs)
    bad[3] = dataclasses.replace(bad[3], table_log_n=tuple(log_n))
    seen = []
    for g in (1, 2, 3):
        group(g)
        with pytest.raises(pg.ProofGenError) as e:
            prove_shard(pg, st, bad, n_workers)
        seen.append((e.value.code, e.value.message))
        root, got = prove_shard(pg, st, irs, n_workers)   # no worker, rider or job of the failed call is left
        assert got == txns and root == roots[5]
    assert seen[0][0] == -3 and "keccak" in seen[0][1]
    assert seen[1] == seen[0] and seen[2] == seen[0]


def test_abort_flag_set_before_the_call(pg, state, reference, group):
    n_workers, st = state
    irs, txns, roots = reference
    flag = C.c_uint8(1)
    for g in (2, 3):
        group(g)
        with pytest.raises(pg.ProofGenError) as e:
            prove_shard(pg, st, irs, n_workers, abort=flag)
        assert e.value.code == -1
    flag.value = 0
    root, got = prove_shard(pg, st, irs[:2], n_workers, abort=flag)
    assert root == roots[2] and got == txns[:2]


def test_a_query_count_that_allows_two_proofs_a_batch_but_not_three(pg, group):
    """stark_num_queries = 100: the query launches index 256 openings, so a batch holds two table proofs.  A group of three
    is split two and one; the bytes are those of txn_group = 1 and nothing is refused."""
    cfg = dict(SMALL_PLONK, stark_num_queries=100)
    st = build_state(pg, cfg, 3)
    try:
        irs = chain(3)
        group(1)
        want = prove_shard(pg, st, irs, 3)
        group(3)
        assert prove_shard(pg, st, irs, 1) == want
        assert prove_shard(pg, st, irs, 3) == want
    finally:
        st.close()
