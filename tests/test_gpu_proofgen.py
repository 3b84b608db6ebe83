"""GPU parity of the reference-shaped API (generate_txn_proof / agg / block, VerifierState) against
the oracle: byte-identical proofs, both verifiers accept, error behaviour of proof_gen.rs."""
import ctypes
import struct

import numpy as np
import pytest

from pg_common import LOG_N, SMALL, WIDTH, ir_words

pytestmark = pytest.mark.gpu


def words(b):
    return np.frombuffer(b, dtype=np.uint64)


@pytest.fixture(scope="module")
def pg(bpg):
    return bpg.proof_gen


@pytest.fixture(scope="module")
def p_state(pg):
    b = pg.ProverStateBuilder()
    for t, name in enumerate(pg.TABLES):
        getattr(b, "set_%s_circuit_size" % name)(range(SMALL["table_log_lo"][t], SMALL["table_log_hi"][t]))
    b.set(**{k: v for k, v in SMALL.items() if not k.startswith("table_")}, n_workers=2, arena_bytes=256 << 20)
    st = b.build()
    yield st
    st.close()


@pytest.fixture(scope="module")
def o_state(oracle):
    return oracle.PgState(**SMALL)


def make_ir(pg, block, txn_before, seed, root=(1, 2, 3, 4), gas=(100, 121), log_n=LOG_N):
    return pg.TxnProofGenIR(block, txn_before, gas[0], gas[1], tuple(root), seed, tuple(log_n), tuple(WIDTH))


@pytest.fixture(scope="module")
def chain(pg, p_state):
    t0 = pg.generate_txn_proof(p_state, make_ir(pg, 7, 0, 0x5EED0001))
    t1 = pg.generate_txn_proof(p_state, make_ir(pg, 7, 1, 0x5EED0002, root=t0.p_vals.state_root_after, gas=(121, 150)))
    t2 = pg.generate_txn_proof(p_state, make_ir(pg, 7, 2, 0x5EED0003, root=t1.p_vals.state_root_after, gas=(150, 150)))
    a01 = pg.generate_agg_proof(p_state, t0, t1)
    a012 = pg.generate_agg_proof(p_state, a01, t2)
    blk = pg.generate_block_proof(p_state, None, a012)
    return t0, t1, t2, a01, a012, blk


def test_txn_agg_block_bytes_match_oracle(pg, p_state, o_state, chain):
    t0, t1, t2, a01, a012, blk = chain
    o0 = o_state.txn(ir_words(7, 0, 0x5EED0001))
    assert (words(t0.intern) == o0).all()
    o1 = o_state.txn(ir_words(7, 1, 0x5EED0002, root_before=t0.p_vals.state_root_after, gas=(121, 150)))
    assert (words(t1.intern) == o1).all()
    oa = o_state.agg(o0, False, o1, False)
    assert (words(a01.intern) == oa).all()
    oa2 = o_state.agg(oa, True, words(t2.intern), False)
    assert (words(a012.intern) == oa2).all()
    ob = o_state.block(None, oa2)
    assert (words(blk.intern) == ob).all()
    assert blk.b_height == 7
    # each side's verifier accepts the other side's proofs
    for p in (t0, a01, a012, blk):
        assert o_state.verify(words(p.intern)) == 0
    v = pg.VerifierState.from_prover_state(p_state)
    v.verify(blk)
    v.verify(ob.tobytes())
    v.verify_any(oa.tobytes())


def test_lock_step_batches_do_not_change_a_byte(pg, p_state, bpg, chain):
    """The seven per-table recursion chains are proved as batches (bp_tune_rec_batch, default 8): whatever the batch
    size -- one proof at a time, uneven splits, all seven at once -- and whichever way the host waits, the txn proof is
    the same bytes (which test_txn_agg_block_bytes_match_oracle pins to the oracle)."""
    t0 = chain[0]
    for n, wait in ((1, 0), (2, 0), (3, 2), (5, 0), (7, 2), (8, 1)):
        with bpg.ops.tuned(rec_batch=n, host_wait=wait):
            again = pg.generate_txn_proof(p_state, make_ir(pg, 7, 0, 0x5EED0001))
        assert again.intern == t0.intern, "batch size %d, host wait mode %d" % (n, wait)


def test_side_lanes_do_not_change_a_byte(pg, bpg, oracle):
    """A prover that is alone on the device spreads its transaction's seven trace commitments over the streams of idle
    workers (bp_tune_side_lanes, csrc/proofgen.cpp SideLane): with three workers to borrow, with none (a state of one
    worker), and with the borrowing switched off the txn proof is the same bytes, and they are the oracle's; two
    transactions at once (at most one of them finds itself alone) agree as well."""
    from concurrent.futures import ThreadPoolExecutor
    want = oracle.PgState(**SMALL).txn(ir_words(7, 0, 0x5EED0001))
    proofs = []
    for n_workers, lanes in ((4, 1), (1, 1), (4, 0)):
        b = pg.ProverStateBuilder()
        for t, name in enumerate(pg.TABLES):
            getattr(b, "set_%s_circuit_size" % name)(range(SMALL["table_log_lo"][t], SMALL["table_log_hi"][t]))
        b.set(**{k: v for k, v in SMALL.items() if not k.startswith("table_")}, n_workers=n_workers, arena_bytes=256 << 20)
        st = b.build()
        try:
            with bpg.ops.tuned(side_lanes=lanes):
                proofs.append(pg.generate_txn_proof(st, make_ir(pg, 7, 0, 0x5EED0001)).intern)
                if n_workers == 4 and lanes:
                    with ThreadPoolExecutor(2) as pool:
                        both = list(pool.map(lambda _: pg.generate_txn_proof(st, make_ir(pg, 7, 0, 0x5EED0001)).intern, range(2)))
                    assert both[0] == both[1] == proofs[-1]
        finally:
            st.close()
    assert proofs[0] == proofs[1] == proofs[2]
    assert (words(proofs[0]) == want).all()


def test_public_values_chain(chain):
    t0, t1, t2, a01, a012, blk = chain
    assert (t0.p_vals.txn_number_before, t0.p_vals.txn_number_after) == (0, 1)
    assert a012.p_vals.txn_number_before == 0 and a012.p_vals.txn_number_after == 3
    assert a012.p_vals.state_root_before == (1, 2, 3, 4)
    assert a012.p_vals.state_root_after == t2.p_vals.state_root_after
    assert a012.p_vals.gas_used_after == 150 and a012.p_vals.block_number == 7


def test_block_proof_chains_to_parent(pg, p_state, chain, o_state):
    *_, a012, blk = chain
    nxt0 = pg.generate_txn_proof(p_state, make_ir(pg, 8, 0, 0x5EED0101))
    nxt1 = pg.generate_txn_proof(p_state, make_ir(pg, 8, 1, 0x5EED0102, root=nxt0.p_vals.state_root_after,
                                                  gas=(121, 130)))
    agg = pg.generate_agg_proof(p_state, nxt0, nxt1)
    b2 = pg.generate_block_proof(p_state, blk, agg)
    assert b2.b_height == 8
    pg.VerifierState.from_prover_state(p_state).verify(b2)
    assert o_state.verify(words(b2.intern)) == 0
    with pytest.raises(pg.ProofGenError) as e:   # height must follow the parent
        pg.generate_block_proof(p_state, b2, agg)
    assert e.value.code == -2


def test_verifier_rejects_corruption(pg, p_state, chain):
    *_, blk = chain
    v = pg.VerifierState.from_prover_state(p_state)
    w = words(blk.intern).copy()
    rng = np.random.default_rng(5)
    for i in list(rng.integers(4, w.size, size=10)) + [4 + 17, 4 + 30 + 16]:  # a public value, the trace cap
        bad = w.copy()
        bad[i] ^= np.uint64(1 << int(rng.integers(0, 60)))
        with pytest.raises(pg.ProofGenError) as e:
            v.verify(bad.tobytes())
        assert e.value.code in (-5, -2)
    with pytest.raises(pg.ProofGenError):        # an agg proof is not a block proof
        v.verify(chain[3].intern)
    with pytest.raises(pg.ProofGenError):
        v.verify(blk.intern[:-8])


def test_agg_requires_contiguous_children(pg, p_state, chain):
    t0, t1, t2, a01, *_ = chain
    with pytest.raises(pg.ProofGenError) as e:
        pg.generate_agg_proof(p_state, t1, t0)
    assert e.value.code == -2 and "contiguous" in e.value.message
    with pytest.raises(pg.ProofGenError):
        pg.generate_agg_proof(p_state, t0, t2)
    with pytest.raises(pg.ProofGenError):        # rhs must follow the whole lhs range
        pg.generate_agg_proof(p_state, a01, t1)


def test_range_and_input_errors(pg, p_state):
    log_n = list(LOG_N)
    log_n[3] = SMALL["table_log_hi"][3]            # one past the configured keccak range
    with pytest.raises(pg.ProofGenError) as e:
        pg.generate_txn_proof(p_state, make_ir(pg, 7, 0, 1, log_n=log_n))
    assert e.value.code == -3 and "keccak" in e.value.message
    with pytest.raises(pg.ProofGenError) as e:
        pg.generate_txn_proof(p_state, b"\x00" * 200)
    assert e.value.code == -2
    with pytest.raises(pg.ProofGenError):
        pg.generate_txn_proof(p_state, b"short")


def test_abort_signal(pg, p_state):
    flag = ctypes.c_int32(1)
    with pytest.raises(pg.ProofGenError) as e:
        pg.generate_txn_proof(p_state, make_ir(pg, 7, 0, 5), abort_signal=flag)
    assert e.value.code == -1
    flag.value = 0
    pg.generate_txn_proof(p_state, make_ir(pg, 7, 0, 5), abort_signal=flag)   # the worker is reusable afterwards
    # the reference's own flag type: Arc<AtomicBool> is one byte (proof_gen.rs:42)
    flag8 = ctypes.c_uint8(1)
    with pytest.raises(pg.ProofGenError) as e:
        pg.generate_txn_proof(p_state, make_ir(pg, 7, 0, 5), abort_signal=flag8)
    assert e.value.code == -1
    flag8.value = 0
    pg.generate_txn_proof(p_state, make_ir(pg, 7, 0, 5), abort_signal=flag8)


def test_concurrent_callers_share_the_state(pg, p_state, o_state):
    from concurrent.futures import ThreadPoolExecutor
    irs = [make_ir(pg, 9, i, 0xABC000 + i) for i in range(6)]
    with ThreadPoolExecutor(4) as ex:
        proofs = list(ex.map(lambda ir: pg.generate_txn_proof(p_state, ir), irs))
    again = pg.generate_txn_proof(p_state, irs[3])
    assert proofs[3].intern == again.intern                  # deterministic, independent of scheduling
    assert (words(proofs[5].intern) == o_state.txn(ir_words(9, 5, 0xABC005))).all()


def test_block_trace_payload_to_block_proof(bpg, pg, p_state):
    """The front door end to end: a trace_protocol JSON payload (combined compact pre-image = one of the
    reference's golden witnesses, five transactions) -> IRs chained like decoding.rs:106-154 -> txn proofs,
    aggregation tree, block proof -> VerifierState::verify."""
    import json
    import os
    from proof_protocol_decoder_amd import trace_protocol as tp
    from proof_protocol_decoder_amd.block_driver import BlockDriver, irs_from_block_trace
    vec = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compact_witness_vectors.json")))
    txns = [{"traces": {"0x" + "%02x" % (17 + i) * 20: {"nonce": hex(i + 1)}},
             "meta": {"byte_code": "0x%04x" % (0xf800 + i), "new_txn_trie_node_byte": "0x01", "new_receipt_trie_node_byte": "0x02",
                      "gas_used": 21000 + i}} for i in range(5)]
    bt = tp.BlockTrace.from_json({"trie_pre_images": {"combined": {"compact": "0x" + vec["complex"][2]["witness_hex"]}},
                                  "txn_info": txns})
    irs = irs_from_block_trace(bt, 9, LOG_N, WIDTH)
    drv = BlockDriver(p_state, n_threads=2)
    try:
        blk = drv.prove_block_distributed(irs)
    finally:
        drv.close()
    assert blk.b_height == 9
    pg.VerifierState.from_prover_state(p_state).verify(blk)
    pv, kind = pg.public_values_of(blk.intern)
    assert kind == 2 and pv.txn_number_before == 0 and pv.txn_number_after == 5
    assert pv.gas_used_after == sum(21000 + i for i in range(5)) and tuple(pv.state_root_before) == irs[0].state_root_before


def test_decoded_block_trace_to_block_proof(bpg, pg, p_state):
    """Front door with the REAL decoder: a block trace whose compact pre-image and
    account traces are replayed natively (minimal tries, deltas, withdrawals: bp_decode_block_trace) -> IRs ->
    txn proofs, aggregation tree, block proof -> VerifierState::verify."""
    import test_decoding as td
    from proof_protocol_decoder_amd import decoding
    from proof_protocol_decoder_amd.block_driver import BlockDriver, irs_from_generation_inputs
    m = td.fresh_model()
    infos = [t for t, _ in td.block(m)]
    other = decoding.OtherBlockData(decoding.BlockLevelData(b"meta", b"hashes", [(td.B, 100)]), b"\x22" * 32)
    gis = decoding.into_txn_proof_gen_ir(td.make_trace(m, infos, hash_out_storage_of=(td.E,)), other)
    irs = irs_from_generation_inputs(gis, 21, LOG_N, WIDTH)
    drv = BlockDriver(p_state, n_threads=2)
    try:
        blk = drv.prove_block_distributed(irs)
    finally:
        drv.close()
    pg.VerifierState.from_prover_state(p_state).verify(blk)
    pv, kind = pg.public_values_of(blk.intern)
    assert kind == 2 and blk.b_height == 21 and (pv.txn_number_before, pv.txn_number_after) == (0, 3)
    assert pv.gas_used_after == 161000 and tuple(pv.state_root_before) == irs[0].state_root_before


def test_decoded_transactions_prove_their_own_keccak_work(bpg, pg, p_state, o_state):
    """GenerationInputs -> the prover, with data instead of a seed for one table: every decoded entry's Keccak table is
    a Keccak-f[1600] trace (AIR 1) of the entry's OWN hashing work -- Keccak-256 of its signed_txn and of its contract
    code (decoding.rs:131-145) -- through bp_generate_txn_proof_keccak.  The witness really is that work (the last
    permutation of the signed transaction ends in its hash), the proofs equal the oracle's byte for byte, the block
    proof verifies."""
    import test_decoding as td
    from proof_protocol_decoder_amd import compact, decoding
    from proof_protocol_decoder_amd.block_driver import (BlockDriver, irs_from_generation_inputs,
                                                         keccak_inputs_of_generation_inputs)
    m = td.fresh_model()
    infos = [t for t, _ in td.block(m)]
    other = decoding.OtherBlockData(decoding.BlockLevelData(b"meta", b"hashes", [(td.B, 100)]), b"\x22" * 32)
    gis = decoding.into_txn_proof_gen_ir(td.make_trace(m, infos, hash_out_storage_of=(td.E,)), other)
    irs = irs_from_generation_inputs(gis, 22, LOG_N, WIDTH, keccak_air=True)
    real = [(g, ir) for g, ir in zip(gis, irs) if g.signed_txn]
    assert real and all(ir.keccak_air and ir.table_width[3] == 2431 for ir in irs)
    g, ir = real[0]
    states = keccak_inputs_of_generation_inputs(g)
    assert [list(x) for x in ir.keccak_inputs] == states and len(states) >= 1
    # the witness is the hashing work: row 24 k + 23 of the trace holds the output of permutation k
    n_txn_perms = len(g.signed_txn) // 136 + 1
    log_n = ir.table_log_n[3]
    inp = np.zeros((((1 << log_n) + 23) // 24, 25), dtype=np.uint64)
    inp[:len(states)] = np.array(states, dtype=np.uint64)
    import torch
    tr = bpg.ops.keccak_trace(log_n, inputs=torch.from_numpy(inp.view(np.int64)).cuda()).cpu().numpy().view(np.uint64)
    r = 24 * (n_txn_perms - 1) + 23
    out = [int(tr[2428, r]) | (int(tr[2429, r]) << 32)] + [int(tr[2314 + 2 * l, r]) | (int(tr[2315 + 2 * l, r]) << 32) for l in (1, 2, 3)]
    assert b"".join(x.to_bytes(8, "little") for x in out) == compact.keccak256(bytes(g.signed_txn))
    # byte parity with the oracle, entry by entry
    for _, e in zip(gis, irs):
        got = pg.generate_txn_proof(p_state, e)
        want = o_state.txn(list(struct.unpack("<25Q", e.to_bytes())), keccak_inputs=np.array(e.keccak_inputs, dtype=np.uint64).reshape(-1, 25))
        assert (words(got.intern) == want).all()
    assert pg.generate_txn_proof(p_state, irs[0], keccak_inputs=()).intern != pg.generate_txn_proof(p_state, irs[0]).intern \
        or not irs[0].keccak_inputs                      # other permutations, another proof
    drv = BlockDriver(p_state, n_threads=2)
    try:
        blk = drv.prove_block_distributed(irs)
    finally:
        drv.close()
    pg.VerifierState.from_prover_state(p_state).verify(blk)
    assert o_state.verify(words(blk.intern)) == 0
    # inputs without the flag, or more permutations than the table has rows for, are refused
    plain = pg.TxnProofGenIR(22, 0, 0, 1, (1, 2, 3, 4), 9, tuple(LOG_N), tuple(WIDTH))
    with pytest.raises(pg.ProofGenError, match="table keccak needs an IR"):
        pg.generate_txn_proof(p_state, plain, keccak_inputs=states)
    with pytest.raises(pg.ProofGenError, match="do not fit"):
        pg.generate_txn_proof(p_state, irs[0], keccak_inputs=[[0] * 25] * 200)


def test_dummy_entries_and_short_blocks(bpg, pg, p_state, o_state):
    """Padding entries (decoding.rs:304-347, 484-520): the dummy IR is proven byte-for-byte like the oracle's, and
    blocks of 0 and 1 transactions -- padded the way the reference pads them -- yield verifying block proofs."""
    from proof_protocol_decoder_amd.block_driver import BlockDriver, pad_with_dummy_irs
    d_ir = pg.TxnProofGenIR(7, 0, 100, 100, (1, 2, 3, 4), 0x44554D4D59000000, tuple(LOG_N), tuple(WIDTH), dummy=True)
    got = pg.generate_txn_proof(p_state, d_ir)
    want_ir = ir_words(7, 0, 0x44554D4D59000000, gas=(100, 100))
    want_ir[1] = 2
    assert (words(got.intern) == o_state.txn(want_ir)).all()
    assert got.p_vals.txn_number_after == 0 and got.p_vals.state_root_after == got.p_vals.state_root_before
    with pytest.raises(ValueError):
        pg.TxnProofGenIR(7, 0, 100, 121, (1, 2, 3, 4), 1, tuple(LOG_N), tuple(WIDTH), dummy=True).to_bytes()
    v = pg.VerifierState.from_prover_state(p_state)
    drv = BlockDriver(p_state, n_threads=2)
    try:
        empty, added = pad_with_dummy_irs([], 11, (5, 6, 7, 8), LOG_N, WIDTH)
        assert added and len(empty) == 2
        blk0 = drv.prove_block_distributed(empty)
        v.verify(blk0)
        pv0, _ = pg.public_values_of(blk0.intern)
        assert (pv0.txn_number_before, pv0.txn_number_after) == (0, 0) and pv0.state_root_after == (5, 6, 7, 8)
        for wd in (False, True):
            one, added = pad_with_dummy_irs([make_ir(pg, 12, 0, 0x5EED0009, root=(5, 6, 7, 8), gas=(0, 21000))], 12,
                                            (5, 6, 7, 8), LOG_N, WIDTH, has_withdrawals=wd)
            assert added and [ir.dummy for ir in one] == ([False, True] if wd else [True, False])
            blk1 = drv.prove_block_distributed(one)
            v.verify(blk1)
            pv1, _ = pg.public_values_of(blk1.intern)
            assert pv1.txn_number_after == 1 and pv1.gas_used_after == 21000 and pv1.state_root_after != (5, 6, 7, 8)
    finally:
        drv.close()


def test_agg_and_block_refuse_children_that_do_not_verify(pg, p_state, chain):
    """prove_aggregation / prove_block verify their children in-circuit (proof_gen.rs:66-75, 97-103); here the same
    check runs on the host before aggregating: a child whose STARK words or public values were tampered with, or
    that claims another circuit, is refused with BP_ERR_VERIFY and nothing is proven on top of it."""
    t0, t1, t2, a01, a012, blk = chain
    w = words(t1.intern).copy()
    w[w.size // 2] ^= np.uint64(4)                         # garbage inside the STARK words
    with pytest.raises(pg.ProofGenError) as e:
        pg.generate_agg_proof(p_state, t0, pg.GeneratedTxnProof(t1.p_vals, w.tobytes()))
    assert e.value.code == -5 and "rhs child" in e.value.message
    # forged public values that still chain (gas_after of the right child): contiguity passes, verification must not
    n_pi = int(words(t1.intern)[2])
    f = words(t1.intern).copy()
    f[4 + n_pi - 13 + 3] += np.uint64(1)
    with pytest.raises(pg.ProofGenError) as e:
        pg.generate_agg_proof(p_state, t0, pg.GeneratedTxnProof(t1.p_vals, f.tobytes()))
    assert e.value.code == -5
    c = words(a01.intern).copy()
    c[3] = 7                                              # an agg container claiming the root circuit
    with pytest.raises(pg.ProofGenError) as e:
        pg.generate_agg_proof(p_state, pg.GeneratedAggProof(a01.p_vals, c.tobytes()), t2)
    assert e.value.code == -5
    g = words(a012.intern).copy()
    g[-5] ^= np.uint64(1)
    with pytest.raises(pg.ProofGenError) as e:
        pg.generate_block_proof(p_state, None, pg.GeneratedAggProof(a012.p_vals, g.tobytes()))
    assert e.value.code == -5
    pb = words(blk.intern).copy()
    pb[-9] ^= np.uint64(1 << 33)
    nxt0 = pg.generate_txn_proof(p_state, make_ir(pg, 8, 0, 0x5EED0101))
    nxt1 = pg.generate_txn_proof(p_state, make_ir(pg, 8, 1, 0x5EED0102, root=nxt0.p_vals.state_root_after, gas=(121, 130)))
    agg = pg.generate_agg_proof(p_state, nxt0, nxt1)
    with pytest.raises(pg.ProofGenError) as e:
        pg.generate_block_proof(p_state, pg.GeneratedBlockProof(7, pb.tobytes()), agg)
    assert e.value.code == -5 and "parent" in e.value.message


def test_decoded_transactions_prove_the_hashing_of_their_partial_tries(bpg, pg, oracle):
    """keccak_trie_nodes=True: the Keccak table of a decoded entry also holds the hashing of its partial tries (state,
    transactions, receipts, storage), node by node -- so the table is taller than the small state's range and this test
    builds a state whose Keccak range reaches 2^10 rows.  The device witness ends the state trie's hashing in the
    entry's pre-state root; proofs equal the oracle's byte for byte; the block verifies."""
    import test_decoding as td
    from proof_protocol_decoder_amd import compact, decoding
    from proof_protocol_decoder_amd.block_driver import BlockDriver, irs_from_generation_inputs
    from proof_protocol_decoder_amd.partial_trie import hashed_node_preimages
    cfg = dict(SMALL, table_log_hi=[*SMALL["table_log_hi"][:3], 11, *SMALL["table_log_hi"][4:]])
    b = pg.ProverStateBuilder()
    for t, name in enumerate(pg.TABLES):
        getattr(b, "set_%s_circuit_size" % name)(range(cfg["table_log_lo"][t], cfg["table_log_hi"][t]))
    b.set(**{k: v for k, v in cfg.items() if not k.startswith("table_")}, n_workers=2, arena_bytes=256 << 20)
    st, ost = b.build(), oracle.PgState(**cfg)
    try:
        m = td.fresh_model()
        infos = [t for t, _ in td.block(m)]
        other = decoding.OtherBlockData(decoding.BlockLevelData(b"meta", b"hashes", [(td.B, 100)]), b"\x22" * 32)
        gis = decoding.into_txn_proof_gen_ir(td.make_trace(m, infos, hash_out_storage_of=(td.E,)), other)
        irs = irs_from_generation_inputs(gis, 23, LOG_N, WIDTH, keccak_air=True, keccak_trie_nodes=True)
        assert max(ir.table_log_n[3] for ir in irs) >= 9
        g, ir = next((g, ir) for g, ir in zip(gis, irs) if g.signed_txn)
        # the permutation that ends the state trie's hashing leaves the pre-state root in the witness
        n_before = len(g.signed_txn) // 136 + 1 + sum(len(c) // 136 + 1 for c in g.contract_code.values())
        k = n_before + sum(len(e) // 136 + 1 for e in hashed_node_preimages(g.tries.state_trie.root)) - 1
        log_n = ir.table_log_n[3]
        inp = np.zeros((((1 << log_n) + 23) // 24, 25), dtype=np.uint64)
        inp[:len(ir.keccak_inputs)] = np.array(ir.keccak_inputs, dtype=np.uint64)
        import torch
        tr = bpg.ops.keccak_trace(log_n, inputs=torch.from_numpy(inp.view(np.int64)).cuda()).cpu().numpy().view(np.uint64)
        r = 24 * k + 23
        out = [int(tr[2428, r]) | (int(tr[2429, r]) << 32)] + [int(tr[2314 + 2 * l, r]) | (int(tr[2315 + 2 * l, r]) << 32) for l in (1, 2, 3)]
        assert b"".join(x.to_bytes(8, "little") for x in out) == g.tries.state_trie.hash()
        for e in irs:
            got = pg.generate_txn_proof(st, e)
            want = ost.txn(list(struct.unpack("<25Q", e.to_bytes())), keccak_inputs=np.array(e.keccak_inputs, dtype=np.uint64).reshape(-1, 25))
            assert (words(got.intern) == want).all()
        drv = BlockDriver(st, n_threads=2)
        try:
            blk = drv.prove_block_distributed(irs)
        finally:
            drv.close()
        pg.VerifierState.from_prover_state(st).verify(blk)
    finally:
        st.close()


def test_decoded_transactions_prove_the_traffic_of_their_hashed_bytes(bpg, pg, oracle):
    """memory_air / byte_packing_air / keccak_sponge_air with keccak_air: four tables of a decoded entry hold data of the
    entry, not a seed -- the Keccak table the hashing of its signed transaction, code and partial tries, the Keccak
    sponge table the absorption of those strings block by block (its xored states are, row for row, the Keccak table's
    permutation inputs), the byte-packing table those bytes taken 32 at a time, the memory table the log of the words
    the chunks spell (written once, read once: the operations the packing rows look up; bp_generate_txn_proof_witness).  The device witnesses contain the bytes; proofs equal the oracle's byte for byte
    (orc_pg_txn_witness); the block verifies."""
    import test_decoding as td
    from proof_protocol_decoder_amd import decoding
    from proof_protocol_decoder_amd.block_driver import (BlockDriver, hashed_preimages_of_generation_inputs,
                                                         irs_from_generation_inputs)
    hi = list(SMALL["table_log_hi"])
    hi[1], hi[3], hi[5], hi[6] = 8, 11, 12, 13
    cfg = dict(SMALL, table_log_hi=hi)
    b = pg.ProverStateBuilder()
    for t, name in enumerate(pg.TABLES):
        getattr(b, "set_%s_circuit_size" % name)(range(cfg["table_log_lo"][t], cfg["table_log_hi"][t]))
    b.set(**{k: v for k, v in cfg.items() if not k.startswith("table_")}, n_workers=2, arena_bytes=256 << 20)
    st, ost = b.build(), oracle.PgState(**cfg)
    try:
        m = td.fresh_model()
        infos = [t for t, _ in td.block(m)]
        other = decoding.OtherBlockData(decoding.BlockLevelData(b"meta", b"hashes", [(td.B, 100)]), b"\x22" * 32)
        gis = decoding.into_txn_proof_gen_ir(td.make_trace(m, infos, hash_out_storage_of=(td.E,)), other)
        irs = irs_from_generation_inputs(gis, 24, LOG_N, WIDTH, keccak_air=True, keccak_trie_nodes=True, memory_air=True,
                                         byte_packing_air=True, keccak_sponge_air=True)
        g, ir = next((g, ir) for g, ir in zip(gis, irs) if g.signed_txn)
        pre = hashed_preimages_of_generation_inputs(g, trie_nodes=True)
        blob = b"".join(pre)
        wit = dict(ir.witness)
        # the device's memory witness of the entry's log holds the hashed bytes (the words its reads return) ...
        import torch
        log_n = ir.table_log_n[6]
        log = np.array(wit[6], dtype=np.uint64).reshape(-1, 11)
        padded = np.zeros((1 << log_n, 11), dtype=np.uint64)
        padded[:len(log)] = log
        last = log[-1].copy()
        last[0] = 1
        for i in range(len(log), 1 << log_n):
            last[2] += np.uint64(1)
            padded[i] = last
        tr = bpg.ops.memory_trace(log_n, inputs=torch.from_numpy(padded.view(np.int64)).cuda()).cpu().numpy().view(np.uint64)
        chunks = [p[o:o + 32] for p in pre for o in range(0, len(p), 32)]
        rd = [i for i in range(len(log)) if tr[0, i] == 1]
        assert len(rd) == len(chunks)
        assert b"".join(sum(int(tr[3 + k, i]) << (32 * k) for k in range(8)).to_bytes(len(c), "big") for i, c in zip(rd, chunks)) == blob
        # ... and the byte-packing witness spells the first chunk of the first string (the signed transaction)
        seqs = np.array(wit[1], dtype=np.uint64).reshape(-1, 6)
        bp = np.zeros((1 << ir.table_log_n[1], 6), dtype=np.uint64)
        bp[:len(seqs)] = seqs
        tb = bpg.ops.byte_packing_trace(ir.table_log_n[1], inputs=torch.from_numpy(bp.view(np.int64)).cuda()).cpu().numpy().view(np.uint64)
        assert sum(int(tb[289 + k, 0]) << (32 * k) for k in range(8)) == int.from_bytes(pre[0][:32], "big")
        assert pre[0] == bytes(g.signed_txn)
        # the sponge rows' permutation inputs (state before ^ block, capacity) are the Keccak table's inputs, row for row
        sp = np.array(wit[4], dtype=np.uint64).reshape(-1, 44)
        xored = sp[:, 19:].copy()
        xored[:, :17] ^= sp[:, 2:19]
        assert (xored == np.array(ir.keccak_inputs, dtype=np.uint64)).all()
        for e in irs:
            got = pg.generate_txn_proof(st, e)
            w = {t: np.array(items, dtype=np.uint64) for t, items in e.witness}
            want = ost.txn(list(struct.unpack("<25Q", e.to_bytes())), keccak_inputs=np.array(e.keccak_inputs, dtype=np.uint64).reshape(-1, 25),
                           witness=w)
            assert (words(got.intern) == want).all()
        # other data, another proof (the sponge rows stay: they and the Keccak-f table are one statement, air::ctl)
        assert pg.generate_txn_proof(st, irs[0], witness={**dict(irs[0].witness), 6: (), 1: ()}).intern != pg.generate_txn_proof(st, irs[0]).intern
        # a seeded sponge table next to the entry's own Keccak-f table cannot be one statement: refused before any proving
        # (round 4 made the seven table proofs first and blamed the tables)
        with pytest.raises(pg.ProofGenError, match="Keccak-f permutations are given but the sponge rows are not") as e:
            pg.generate_txn_proof(st, ir, witness={6: (), 1: ()})
        assert e.value.code == -2
        # the library's own front door for decoded entries (csrc/gi.cpp): bp_generate_txn_proof_gi derives the same IR and
        # the same four witnesses from the "BPGGENI1" bytes, entry by entry along the chain -- same proof bytes --, and
        # bp_prove_shard_gi proves the whole slice and its tree
        from proof_protocol_decoder_amd.block_driver import GiOptions, generate_txn_proof_gi, gi_chain_start, gi_irs
        geni = decoding.generation_inputs_bytes(td.make_trace(m, infos, hash_out_storage_of=(td.E,)), other)
        opts = GiOptions.make(24, LOG_N, WIDTH, keccak_air=True, keccak_trie_nodes=True, memory_air=True, byte_packing_air=True,
                              keccak_sponge_air=True)
        assert gi_irs(geni, opts) == [x.to_bytes() for x in irs]
        chain = gi_chain_start(geni)
        by_entry = [generate_txn_proof_gi(st, geni, k, opts, chain) for k in range(len(irs))]
        assert [p.intern for p in by_entry] == [pg.generate_txn_proof(st, x).intern for x in irs]
        assert chain.txn_number == by_entry[-1].p_vals.txn_number_after and chain.gas_used == by_entry[-1].p_vals.gas_used_after
        # BP_GI_LOGIC_AIR: the entry's logic table by its AIR too; its first rows are the sponge rows' XORs, derived inside
        # the library from the sponge table's trace (keccak_sponge -> logic), the table grown to hold five per sponge row
        opts_l = GiOptions.make(24, LOG_N, WIDTH, keccak_air=True, keccak_trie_nodes=True, memory_air=True, byte_packing_air=True,
                                keccak_sponge_air=True, logic_air=True)
        irs_l = irs_from_generation_inputs(gis, 24, LOG_N, WIDTH, keccak_air=True, keccak_trie_nodes=True, memory_air=True,
                                           byte_packing_air=True, keccak_sponge_air=True, logic_air=True)
        assert gi_irs(geni, opts_l) == [x.to_bytes() for x in irs_l]
        assert all(x.table_width[5] == 524 and (1 << x.table_log_n[5]) >= (5 << x.table_log_n[4]) for x in irs_l)
        chain_l = gi_chain_start(geni)
        for k, e in enumerate(irs_l[:2]):
            got = generate_txn_proof_gi(st, geni, k, opts_l, chain_l)
            w = {t: np.array(items, dtype=np.uint64) for t, items in e.witness}
            want = ost.txn(list(struct.unpack("<25Q", e.to_bytes())), keccak_inputs=np.array(e.keccak_inputs, dtype=np.uint64).reshape(-1, 25),
                           witness=w)
            assert (words(got.intern) == want).all()
        drv2 = BlockDriver(st, n_threads=2)
        try:
            top, leaves = drv2.prove_shard_gi(geni, 0, len(irs), opts)
            assert [p.intern for p in leaves] == [p.intern for p in by_entry]
            want_top, _ = drv2.prove_shard(irs)       # the Python-side IRs through bp_run_shard: the same tree, the same bytes
            assert top.intern == want_top.intern
        finally:
            drv2.close()
        drv = BlockDriver(st, n_threads=2)
        try:
            blk = drv.prove_block_distributed(irs)
        finally:
            drv.close()
        pg.VerifierState.from_prover_state(st).verify(blk)
        # caller-given data is CHECKED (the CPU verifier runs on the table proof just made): a log whose read returns
        # something else than what was written, or sponge rows that do not chain, end the call
        bad_log = [list(r) for r in wit[6]]
        k = next(i for i, r in enumerate(bad_log) if r[0] == 1)
        bad_log[k][3] ^= 1
        with pytest.raises(pg.ProofGenError, match="memory does not satisfy its AIR") as e:
            pg.generate_txn_proof(st, ir, witness={**wit, 6: bad_log})
        assert e.value.code == -5
        if len(wit[4]) >= 2:
            bad_rows = [list(r) for r in wit[4]]
            k = next(i for i, r in enumerate(bad_rows) if r[0] == 1)     # a full block: the next row continues from it
            bad_rows[k + 1][19 + 3] ^= 1
            with pytest.raises(pg.ProofGenError, match="keccak_sponge does not satisfy its AIR"):
                pg.generate_txn_proof(st, ir, witness={**wit, 4: bad_rows})
        # data for a table whose IR flag is not set is refused
        plain = pg.TxnProofGenIR(9, 0, 0, 21000, (1, 2, 3, 4), 5, tuple(LOG_N), tuple(WIDTH))
        with pytest.raises(pg.ProofGenError, match="memory"):
            pg.generate_txn_proof(st, plain, witness={6: ()})
    finally:
        st.close()


def test_txn_with_a_real_keccak_table_matches_the_oracle(pg, p_state, o_state):
    """IR flag 0x100: the Keccak table of the transaction (index 3, prover_state.rs:85-93) is a real Keccak-f[1600]
    trace proven with AIR 1 (2431 columns, witness drawn from the seed) next to six synthetic tables.  Byte parity of
    the txn proof with the oracle, aggregation with an ordinary txn, block proof accepted by both verifiers."""
    width = list(WIDTH)
    width[3] = 2431
    ir0 = pg.TxnProofGenIR(9, 0, 0, 21000, (1, 2, 3, 4), 0x5EED0010, tuple(LOG_N), tuple(width), keccak_air=True)
    t0 = pg.generate_txn_proof(p_state, ir0)
    iw = list(struct.unpack("<25Q", ir0.to_bytes()))
    assert iw[1] == 0x101 and iw[18 + 3] == 2431
    want = o_state.txn(iw)
    assert (words(t0.intern) == want).all()
    plain = pg.TxnProofGenIR(9, 0, 0, 21000, (1, 2, 3, 4), 0x5EED0010, tuple(LOG_N), tuple(width))
    assert pg.generate_txn_proof(p_state, plain).intern != t0.intern          # the same table proven with AIR 0 differs
    t1 = pg.generate_txn_proof(p_state, make_ir(pg, 9, 1, 0x5EED0011, root=t0.p_vals.state_root_after, gas=(21000, 42000)))
    blk = pg.generate_block_proof(p_state, None, pg.generate_agg_proof(p_state, t0, t1))
    pg.VerifierState.from_prover_state(p_state).verify(blk)
    assert o_state.verify(words(blk.intern)) == 0
    with pytest.raises(pg.ProofGenError, match="2431"):                        # the AIR's width is not negotiable
        pg.TxnProofGenIR(9, 0, 0, 21000, (1, 2, 3, 4), 1, tuple(LOG_N), tuple(WIDTH), keccak_air=True).to_bytes()


def test_txn_with_six_real_tables_matches_the_oracle(pg, p_state, o_state):
    """IR flags 0x800 | 0x1000 | 0x100 | 0x2000 | 0x200 | 0x400: the arithmetic (index 0), byte-packing (1), Keccak (3),
    Keccak sponge (4), logic (5) and memory (6) tables of the transaction are proven with AIR 4, 5, 1, 6, 2 and 3; only
    the CPU table (2) stays synthetic.  Byte parity with the oracle; the block verifies."""
    width = list(WIDTH)
    width[0], width[1], width[3], width[4], width[5], width[6] = 309, 299, 2431, 2414, 524, 45
    ir0 = pg.TxnProofGenIR(9, 0, 0, 21000, (1, 2, 3, 4), 0x5EED0020, tuple(LOG_N), tuple(width), keccak_air=True, logic_air=True,
                           memory_air=True, arithmetic_air=True, byte_packing_air=True, keccak_sponge_air=True)
    t0 = pg.generate_txn_proof(p_state, ir0)
    iw = list(struct.unpack("<25Q", ir0.to_bytes()))
    assert iw[1] == 0x3F01 and iw[18 + 0] == 309 and iw[18 + 1] == 299 and iw[18 + 4] == 2414 and iw[18 + 5] == 524 and iw[18 + 6] == 45
    assert (words(t0.intern) == o_state.txn(iw)).all()
    only_logic = pg.TxnProofGenIR(9, 0, 0, 21000, (1, 2, 3, 4), 0x5EED0020, tuple(LOG_N), (*WIDTH[:5], 524, WIDTH[6]), logic_air=True)
    t_l = pg.generate_txn_proof(p_state, only_logic)
    iw_l = list(struct.unpack("<25Q", only_logic.to_bytes()))
    assert iw_l[1] == 0x201 and (words(t_l.intern) == o_state.txn(iw_l)).all() and t_l.intern != t0.intern
    # the arithmetic table by the multiplication AIR instead (AIR 7, flag 0x4000): seeded products, and the caller's
    mul_ir = pg.TxnProofGenIR(9, 0, 0, 21000, (1, 2, 3, 4), 0x5EED0027, tuple(LOG_N), (1217, *WIDTH[1:]), arithmetic_mul_air=True)
    iw_m = list(struct.unpack("<25Q", mul_ir.to_bytes()))
    t_m = pg.generate_txn_proof(p_state, mul_ir)
    assert iw_m[1] == 0x4001 and (words(t_m.intern) == o_state.txn(iw_m)).all()
    ops = ((1, 7, 0, 0, 0, 9, 0, 0, 0), (1, 2**64 - 1, 5, 2**63, 1, 3, 2**64 - 2, 0, 2**62))
    t_m2 = pg.generate_txn_proof(p_state, mul_ir, witness={0: ops})
    assert (words(t_m2.intern) == o_state.txn(iw_m, witness={0: np.array(ops, dtype=np.uint64)})).all() and t_m2.intern != t_m.intern
    t1 = pg.generate_txn_proof(p_state, make_ir(pg, 9, 1, 0x5EED0021, root=t0.p_vals.state_root_after, gas=(21000, 42000)))
    blk = pg.generate_block_proof(p_state, None, pg.generate_agg_proof(p_state, t0, t1))
    pg.VerifierState.from_prover_state(p_state).verify(blk)
    assert o_state.verify(words(blk.intern)) == 0
    with pytest.raises(pg.ProofGenError, match="524"):                         # the AIR's width is not negotiable
        pg.TxnProofGenIR(9, 0, 0, 21000, (1, 2, 3, 4), 1, tuple(LOG_N), tuple(WIDTH), logic_air=True).to_bytes()
    with pytest.raises(pg.ProofGenError, match="45"):
        pg.TxnProofGenIR(9, 0, 0, 21000, (1, 2, 3, 4), 1, tuple(LOG_N), tuple(WIDTH), memory_air=True).to_bytes()
    with pytest.raises(pg.ProofGenError, match="309"):
        pg.TxnProofGenIR(9, 0, 0, 21000, (1, 2, 3, 4), 1, tuple(LOG_N), tuple(WIDTH), arithmetic_air=True).to_bytes()
    with pytest.raises(pg.ProofGenError, match="299"):
        pg.TxnProofGenIR(9, 0, 0, 21000, (1, 2, 3, 4), 1, tuple(LOG_N), tuple(WIDTH), byte_packing_air=True).to_bytes()
    with pytest.raises(pg.ProofGenError, match="2414"):
        pg.TxnProofGenIR(9, 0, 0, 21000, (1, 2, 3, 4), 1, tuple(LOG_N), tuple(WIDTH), keccak_sponge_air=True).to_bytes()


def test_table_proofs_and_their_lookups_match_the_oracle(pg, p_state, o_state, oracle):
    """bp_generate_txn_table_proofs = upstream's `prove` before the recursion (AllProof): the seven table proofs on one
    transcript.  With six real tables the sponge table's rows look their permutations up in the Keccak-f table and the
    byte-packing table's words are operations of the memory table (csrc/air.hpp namespace ctl): bytes equal the oracle's (oracle/ctl.c states the lookup columns independently), both
    verifiers accept both provers' output, and the prover refuses tables that are valid alone but not one statement."""
    width = list(WIDTH)
    width[0], width[1], width[3], width[4], width[5], width[6] = 309, 299, 2431, 2414, 524, 45
    ir0 = pg.TxnProofGenIR(9, 0, 0, 21000, (1, 2, 3, 4), 0x5EED0C71, tuple(LOG_N), tuple(width), keccak_air=True, logic_air=True,
                           memory_air=True, arithmetic_air=True, byte_packing_air=True, keccak_sponge_air=True)
    iw = list(struct.unpack("<25Q", ir0.to_bytes()))
    got = pg.generate_txn_table_proofs(p_state, ir0)
    want = o_state.txn_tables(iw)
    assert (words(got) == want).all()
    pg.verify_txn_table_proofs(p_state.cfg, got)
    assert o_state.verify_tables(words(got)) == 0
    # the lookup is not vacuous (see tests/test_lookups.py for the layout): the sponge table's product is not 1
    from test_lookups import first_row_openings
    looking, looked = first_row_openings(oracle, words(got), 4), first_row_openings(oracle, words(got), 3)
    assert (looking[0] == looked[2]).all() and (looking[1] == looked[3]).all() and tuple(looking[0]) != (1, 0)
    # caller-given tables: three messages absorbed by the sponge table, their permutations in the Keccak-f table
    from test_lookups import sponge_and_keccak_work
    rows, perms = sponge_and_keccak_work(oracle, [b"abc", bytes(range(200)), b""])
    w2 = list(WIDTH)
    w2[3], w2[4] = 2431, 2414
    ir1 = pg.TxnProofGenIR(9, 0, 0, 21000, (1, 2, 3, 4), 0x5EED0C72, tuple(LOG_N), tuple(w2), keccak_air=True, keccak_sponge_air=True)
    iw1 = list(struct.unpack("<25Q", ir1.to_bytes()))
    got1 = pg.generate_txn_table_proofs(p_state, ir1, witness={3: perms, 4: rows})
    assert (words(got1) == o_state.txn_tables(iw1, witness={3: perms, 4: rows})).all()
    assert o_state.verify_tables(words(got1)) == 0
    assert (words(pg.generate_txn_proof(p_state, ir1, witness={3: perms, 4: rows}).intern)
            == o_state.txn(iw1, witness={3: np.array(perms, dtype=np.uint64), 4: np.array(rows, dtype=np.uint64)})).all()
    # one lane of one permutation differs: each table is valid alone, together they are not one statement
    bad = [list(p) for p in perms]
    bad[1][7] ^= 1 << 33
    for call in (pg.generate_txn_table_proofs, pg.generate_txn_proof):
        with pytest.raises(pg.ProofGenError, match="cross-table lookup keccak_sponge -> keccak_f does not hold") as e:
            call(p_state, ir1, witness={3: bad, 4: rows})
        assert e.value.code == -5
    # the verifier of the one side refuses what the other side's prover made of the bad tables
    oracle.lib().orc_pg_set_prover_lookup_check(0)
    try:
        bad_tp = o_state.txn_tables(iw1, witness={3: bad, 4: rows})
    finally:
        oracle.lib().orc_pg_set_prover_lookup_check(1)
    with pytest.raises(pg.ProofGenError, match="cross-table lookup"):
        pg.verify_txn_table_proofs(p_state.cfg, bad_tp.tobytes())
    # the second lookup, byte_packing -> memory: in the six-table transaction above the packing rows' words are the
    # operations the (seeded) memory table exposes ...
    packing, memory = first_row_openings(oracle, words(got), 1), first_row_openings(oracle, words(got), 6)
    assert (packing[0] == memory[0]).all() and (packing[1] == memory[1]).all() and tuple(packing[0]) != (1, 0)
    # ... and with caller-given tables: the strings' chunks and the log of the words they spell
    from proof_protocol_decoder_amd.block_driver import memory_and_byte_packing_work_of_preimages
    log, seqs = memory_and_byte_packing_work_of_preimages([b"hello, memory", bytes(range(70)), b"x" * 32])
    w3 = list(WIDTH)
    w3[1], w3[6] = 299, 45
    ir2 = pg.TxnProofGenIR(9, 0, 0, 21000, (1, 2, 3, 4), 0x5EED0C73, tuple(LOG_N), tuple(w3), byte_packing_air=True, memory_air=True)
    iw2 = list(struct.unpack("<25Q", ir2.to_bytes()))
    got2 = pg.generate_txn_table_proofs(p_state, ir2, witness={1: seqs, 6: log})
    assert (words(got2) == o_state.txn_tables(iw2, witness={1: seqs, 6: log})).all()
    assert o_state.verify_tables(words(got2)) == 0
    bad_seqs = [list(x) for x in seqs]
    bad_seqs[1][2] ^= 0x40   # one byte of one chunk: still a sequence, still a memory -- of another word
    for call in (pg.generate_txn_table_proofs, pg.generate_txn_proof):
        with pytest.raises(pg.ProofGenError, match="cross-table lookup byte_packing -> memory does not hold") as e:
            call(p_state, ir2, witness={1: bad_seqs, 6: log})
        assert e.value.code == -5


S1_LOG_N = (16, 9, 12, 14, 9, 12, 17)
S1_WIDTH = (128, 128, 192, 2432, 512, 320, 16)


def _sha(b):
    import hashlib
    return hashlib.sha256(bytes(b)).hexdigest()


def test_block16_at_default_config_matches_golden(bpg, pg, oracle):
    """BASELINE configs[1]: a 16-txn synthetic block of S1 (transfer-txn sized) transactions through L1 at
    bp_config_default parameters (standard_fast_config: 84 queries, 16 PoW bits; recursion shape 2^13 x 135, 28
    queries; default table ranges of constants.rs:6-18), one GPU.  Byte parity: txn proofs 0, 1 and 15, the
    aggregation of 0 and 1 and the block proof of {0, 1} equal the oracle's (digests made in the build container by
    tools/gen_hotpath_golden.py); the 16-txn block proof from BlockDriver.prove_block_distributed is accepted by
    both verifiers."""
    import json
    import os
    from proof_protocol_decoder_amd.block_driver import BlockDriver, synthetic_block_irs
    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hotpath_golden.json")))["block16"]
    st = pg.ProverStateBuilder().set(n_workers=8, arena_bytes=5 << 30).build()
    try:
        irs = synthetic_block_irs(gold["block_number"], 16, S1_LOG_N, S1_WIDTH)
        assert list(struct.unpack("<25Q", irs[15].to_bytes())) == gold["ir15"]     # the chain the oracle was given
        drv = BlockDriver(st, n_threads=8)
        try:
            top, txns = drv.prove_shard(irs)
            blk = drv.prove_block_distributed(irs)
        finally:
            drv.close()
        for i in (0, 1, 15):
            assert words(txns[i].intern).size == gold["txn%d" % i]["n_words"]
            assert _sha(txns[i].intern) == gold["txn%d" % i]["sha256"], "txn %d differs from the oracle's proof" % i
        a01 = pg.generate_agg_proof(st, txns[0], txns[1])
        assert _sha(a01.intern) == gold["agg_0_1"]["sha256"]
        b01 = pg.generate_block_proof(st, None, a01)
        assert _sha(b01.intern) == gold["block_of_0_1"]["sha256"]
        pv, kind = pg.public_values_of(blk.intern)
        assert kind == 2 and (pv.txn_number_before, pv.txn_number_after) == (0, 16) and pv.gas_used_after == 16 * 21000
        assert pv.state_root_after == txns[15].p_vals.state_root_after and blk.b_height == gold["block_number"]
        assert blk.intern == pg.generate_block_proof(st, None, top).intern           # same tree either way
        # the WHOLE block, byte for byte: the oracle proved all 16 txns, the 15 aggregations and the block proof once
        # on the GPU box's host cores (tools/gen_block16_golden.py)
        full = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hotpath_golden.json")))["block16_full"]
        assert [_sha(t.intern) for t in txns] == full["txn_sha256"]
        assert _sha(blk.intern) == full["block_sha256"] and words(blk.intern).size == full["block_words"]
        pg.VerifierState.from_prover_state(st).verify(blk)
        ost = oracle.PgState(table_log_lo=list(S1_LOG_N), table_log_hi=[x + 1 for x in S1_LOG_N], stark_rate_bits=1,
                             stark_cap_height=4, stark_num_queries=84, stark_pow_bits=16, arity_bits=4, final_poly_bits=5,
                             rec_log_n=13, rec_n_cols=135, rec_n_const=85, rec_rate_bits=3, rec_num_queries=28,
                             rec_pow_bits=16, shrink_depth=3, rec_air_id=8)
        assert ost.verify(words(blk.intern)) == 0
        assert ost.verify(words(txns[7].intern)) == 0
    finally:
        st.close()


def test_closing_a_state_after_a_table_proof_parked_a_worker_does_not_hang():
    """Found in round 3: bp_stark_prove_air leaves a parked worker on the device; when the first bp_state_build then
    switched the device to blocking host waits, the hipFree of bp_state_free never returned.  The wait mode is now
    fixed before the library's first stream.  Fresh process (the order of calls in the process is the point)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "hang_probe.py"), "s"], capture_output=True, text=True,
                       timeout=300, cwd=root, env=dict(os.environ, WD="120"))
    assert r.returncode == 0 and "state closed" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
    assert "host wait mode 1" in r.stdout   # the library came first: host waits sleep


def test_a_device_the_process_already_used_keeps_its_wait_mode():
    """Found in round 3 (tests/test_gpu_kernels.py followed directly by tests/test_gpu_stark.py): when the process
    had already run kernels on the device (torch, L0 entry points on the null stream) before the library's first
    worker, switching the device to blocking host waits made the first hipFree after it wait forever
    (hip::Device::SyncAllStreams on the older queues).  bp_use_blocking_sync now leaves a device in use alone."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "hang_probe.py"), "ts"], capture_output=True, text=True,
                       timeout=300, cwd=root, env=dict(os.environ, WD="120"))
    assert r.returncode == 0 and "state closed" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
    assert "host wait mode 2" in r.stdout


def test_state_build_reports_too_few_hardware_queues_and_the_wait_mode():
    """bp_state_warnings: the one run-time prerequisite of a multi-stream state that the library cannot set itself
    (GPU_MAX_HW_QUEUES is read when the HIP runtime starts) is checked at bp_state_build and reported as text; so is
    the host-wait mode of a device the process used first.  Fresh processes: both are per-process facts."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(steps, queues):
        env = dict(os.environ, WD="120")
        env.pop("GPU_MAX_HW_QUEUES", None)
        if queues:
            env["GPU_MAX_HW_QUEUES"] = queues
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "hang_probe.py"), steps], capture_output=True,
                           text=True, timeout=300, cwd=root, env=env)
        assert r.returncode == 0 and "state closed" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
        return [l for l in r.stdout.splitlines() if "state warnings:" in l][0]
    low = run("x", "1")          # the probe's state has two prover streams
    assert "GPU_MAX_HW_QUEUES is 1 but this state has 2 prover streams" in low and "poll-and-sleep" not in low
    assert run("x", "8").endswith("state warnings: none")
    used = run("t", "8")         # torch first: mode 2, reported; enough queues: not reported
    assert "GPU_MAX_HW_QUEUES" not in used and "poll-and-sleep" in used


RCCL_CHILD = r'''
import os, sys
sys.path.insert(0, {root!r})
os.environ.setdefault("GPU_MAX_HW_QUEUES", "32")
import torch, torch.distributed as dist
import proof_protocol_decoder_amd as pkg
from proof_protocol_decoder_amd import proof_gen as pg
from proof_protocol_decoder_amd.block_driver import BlockDriver, TorchGather, synthetic_block_irs
sys.path.insert(0, os.path.join({root!r}, "tests"))
from pg_common import LOG_N, SMALL, WIDTH
rank, local_rank, world = int(os.environ["RANK"]), int(os.environ["LOCAL_RANK"]), int(os.environ["WORLD_SIZE"])
pkg.lib().bp_use_blocking_sync(local_rank)
torch.cuda.set_device(local_rank)
dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))      # bench.py's exact branch
dev = torch.device("cuda", local_rank)
b = pg.ProverStateBuilder()
for t, name in enumerate(pg.TABLES):
    getattr(b, "set_%s_circuit_size" % name)(range(SMALL["table_log_lo"][t], SMALL["table_log_hi"][t]))
b.set(**{{k: v for k, v in SMALL.items() if not k.startswith("table_")}}, device=local_rank, n_workers=2, arena_bytes=256 << 20)
st = b.build()
drv = BlockDriver(st, n_threads=2)
irs = synthetic_block_irs(31, 4, LOG_N, WIDTH)
dist.barrier(); torch.cuda.synchronize()
blk = drv.prove_block_distributed(irs, rank, world, TorchGather(dev))
torch.cuda.synchronize(); dist.barrier()
t = torch.tensor([1.25 + rank], dtype=torch.float64, device=dev)
dist.all_reduce(t, op=dist.ReduceOp.MAX)                                          # bench.py's max-over-ranks timing
assert abs(t.item() - (1.25 + world - 1)) < 1e-9
raws = TorchGather(dev).gather_bytes(b"rank%d" % rank)
if rank == 0:
    assert raws == [b"rank%d" % r for r in range(world)]
    pg.VerifierState.from_prover_state(st).verify(blk)
    pv, kind = pg.public_values_of(blk.intern)
    assert kind == 2 and pv.txn_number_after == 4
    print("RCCL_PATH_OK backend=%s world=%d" % (dist.get_backend(), world))
drv.close(); st.close()
dist.destroy_process_group()
'''


def test_rccl_branch_of_the_bench_runs_at_world_size_1(tmp_path):
    """bench.py's multi-GPU branch -- init_process_group("nccl", device_id=...), TorchGather on a cuda device
    (all_gather of lengths + padded uint8 gather), all_reduce(MAX) -- executed for real on the one GPU this box
    has: a fresh child process under torch.distributed.run (started before it touches the GPU), world size 1,
    4-txn block, block proof verified.  The 8-GPU curve itself is the driver's to measure."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "rccl_child.py"
    script.write_text(RCCL_CHILD.format(root=root))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                        "--master-addr", "127.0.0.1", "--master-port", "29733", str(script)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "RCCL_PATH_OK backend=nccl world=1" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
