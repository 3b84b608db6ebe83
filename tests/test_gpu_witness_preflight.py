"""The transaction witness pre-flight (bp_check_txn_witness, proof_gen.check_txn_witness) on a decoded entry whose four
tables hold the entry's own data (the setup of test_gpu_proofgen.py's
test_decoded_transactions_prove_the_traffic_of_their_hashed_bytes): it agrees with generate_txn_proof on the status of
every input and names the table and row, or the lookup and its first unmatched row, without proving anything."""
import pytest

from pg_common import LOG_N, SMALL, WIDTH

pytestmark = pytest.mark.gpu
VERIFY, INVALID = -5, -2


@pytest.fixture(scope="module")
def entry(bpg):
    import test_decoding as td
    from proof_protocol_decoder_amd import decoding, proof_gen as pg
    from proof_protocol_decoder_amd.block_driver import irs_from_generation_inputs
    hi = list(SMALL["table_log_hi"])
    hi[1], hi[3], hi[5], hi[6] = 8, 11, 12, 13
    cfg = dict(SMALL, table_log_hi=hi)
    b = pg.ProverStateBuilder()
    for t, name in enumerate(pg.TABLES):
        getattr(b, "set_%s_circuit_size" % name)(range(cfg["table_log_lo"][t], cfg["table_log_hi"][t]))
    b.set(**{k: v for k, v in cfg.items() if not k.startswith("table_")}, n_workers=2, arena_bytes=256 << 20)
    st = b.build()
    m = td.fresh_model()
    infos = [t for t, _ in td.block(m)]
    other = decoding.OtherBlockData(decoding.BlockLevelData(b"meta", b"hashes", [(td.B, 100)]), b"\x22" * 32)
    gis = decoding.into_txn_proof_gen_ir(td.make_trace(m, infos, hash_out_storage_of=(td.E,)), other)
    irs = irs_from_generation_inputs(gis, 24, LOG_N, WIDTH, keccak_air=True, keccak_trie_nodes=True, memory_air=True,
                                     byte_packing_air=True, keccak_sponge_air=True)
    ir = next(ir for g, ir in zip(gis, irs) if g.signed_txn)
    yield pg, st, ir, dict(ir.witness)
    st.close()


def prover_status(pg, st, ir, witness):
    try:
        pg.generate_txn_proof(st, ir, witness=witness)
        return 0, ""
    except pg.ProofGenError as e:
        return e.code, e.message


def test_the_good_witness_passes(entry):
    pg, st, ir, wit = entry
    rep = pg.check_txn_witness(st, ir)
    assert rep.ok, rep.message
    for t in (1, 3, 4, 6):
        assert rep.table[t].checked and rep.table[t].n_violated_rows == 0, t
    assert rep.table[4].given and rep.table[6].given
    for i in (0, 1):    # keccak_sponge -> keccak_f, byte_packing -> memory (the logic table is synthetic here)
        lk = rep.lookup[i]
        assert lk.checked and lk.holds and lk.n_looking == lk.n_looked > 0 and lk.first_looking_row == lk.first_looked_row == -1
    assert not rep.lookup[2].checked
    assert prover_status(pg, st, ir, None)[0] == 0


def test_a_stale_memory_read_is_named_at_its_row(entry):
    pg, st, ir, wit = entry
    bad_log = [list(r) for r in wit[6]]
    k = next(i for i, r in enumerate(bad_log) if r[0] == 1)
    bad_log[k][3] ^= 1
    w = {**wit, 6: bad_log}
    rep = pg.check_txn_witness(st, ir, witness=w)
    assert rep.status == VERIFY and "memory does not satisfy its AIR" in rep.message
    rows = {v.row for v in rep.violations(6)}
    assert rows and rows <= {k - 1, k} and rep.table[6].n_violated_rows >= 1
    code, msg = prover_status(pg, st, ir, w)
    assert code == VERIFY and "memory does not satisfy its AIR" in msg


def test_broken_sponge_chaining_is_named_at_its_row(entry):
    pg, st, ir, wit = entry
    if len(wit[4]) < 2:
        pytest.skip("the entry absorbs one block")
    bad_rows = [list(r) for r in wit[4]]
    k = next(i for i, r in enumerate(bad_rows) if r[0] == 1)
    bad_rows[k + 1][19 + 3] ^= 1
    w = {**wit, 4: bad_rows}
    rep = pg.check_txn_witness(st, ir, witness=w)
    assert rep.status == VERIFY and "keccak_sponge does not satisfy its AIR" in rep.message
    assert {v.row for v in rep.violations(4)} <= {k, k + 1} and rep.table[4].n_violated_rows >= 1
    assert prover_status(pg, st, ir, w)[0] == VERIFY


def test_a_sequence_that_spells_another_word_breaks_the_lookup(entry):
    pg, st, ir, wit = entry
    seqs = [list(r) for r in wit[1]]
    seqs[0][2] ^= 1                     # byte slot 0 of the first sequence: a valid packing row, but another word
    w = {**wit, 1: seqs}
    rep = pg.check_txn_witness(st, ir, witness=w)
    assert rep.status == VERIFY and "byte_packing -> memory does not hold" in rep.message, rep.message
    lk = rep.lookup[1]
    assert lk.checked and not lk.holds and lk.first_looking_row == 0 and lk.first_looked_row >= 0
    assert rep.table[1].n_violated_rows == 0 and rep.table[6].n_violated_rows == 0
    code, msg = prover_status(pg, st, ir, w)
    assert code == VERIFY and "byte_packing -> memory does not hold" in msg


def test_sponge_rows_not_given_is_the_provers_refusal(entry):
    pg, st, ir, wit = entry
    with pytest.raises(pg.ProofGenError, match="Keccak-f permutations are given but the sponge rows are not") as e:
        pg.check_txn_witness(st, ir, witness={6: (), 1: ()})
    assert e.value.code == INVALID
    assert prover_status(pg, st, ir, {6: (), 1: ()})[0] == INVALID
