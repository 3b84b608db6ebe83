"""The edge tables of tests/witness_edges.py proven on the CPU, before any device generator is held against them: the
oracle's trace of every table equals the Python-integer model on every modelled column; the product's host checker
finds a valid table clean and rejects exactly the rows the model names (which are also the oracle's rows); the valid
memory log reaches every gap bit; an oracle proof of every valid table is accepted by both verifiers.  GPU side:
tests/test_gpu_witness_edges.py."""
import hashlib

import numpy as np
import pytest

import witness_edges as we
from air_check_util import oracle_violated_rows
from builtin_airs import AIRS, keccak, product_verify, prove

TABLES = we.all_tables()
IDS = [t.name for t in TABLES]


def oracle_trace(oracle, table):
    return oracle.air_trace(table.air_id, table.log_n, inputs=table.inputs)


def host_rows(table, trace):
    import proof_protocol_decoder_amd as pkg
    n = trace.shape[1]
    res = pkg.ops.check_air_trace_host(table.air_id, trace, max_rows=n)
    assert res.n_violated_rows == len(res.rows)
    return set(res.rows)


def test_the_keccak_model_is_keccak():
    """the Keccak-f the AIR 1 and AIR 6 models are written on, against hashlib"""
    def permute(st):
        return np.array(we.keccak_f(st), dtype=np.uint64)
    for msg in (b"", b"abc", b"q" * 135, b"r" * 136, b"witness edges" * 30):
        assert keccak.sha3_256_by_hand(permute, msg)[0] == hashlib.sha3_256(msg).digest()
    assert we.keccak_f([0] * 25)[:2] == [0xF1258F7940E1DDE7, 0x84D5CCF933C0478A]


def test_tables_hold_the_edges():
    assert sorted({t.air_id for t in TABLES}) == [1, 2, 3, 4, 5, 6, 7]
    for t in TABLES:
        assert 4 <= t.log_n <= 7 and t.kind in (we.VALID, we.FALSE, we.OUTSIDE)
    kinds = [(t.air_id, t.kind) for t in TABLES]
    assert kinds.count((3, we.FALSE)) == 3 and (3, we.OUTSIDE) in kinds and (6, we.OUTSIDE) in kinds
    assert [k for a, k in kinds if a not in (3, 6)] == [we.VALID] * 5
    bp = next(t for t in TABLES if t.air_id == 5)
    assert {int(v) & 0xFF for v in bp.inputs[:, 1]} == set(we.BP_LENGTHS)
    # the carries of AIR 7: no operands produce more than (2^256 - 1)^2 does, column by column, and bit 20 stays zero
    top, _ = we.mul_carries(we.M - 1, we.M - 1)
    assert max(top) == top[15] == we.MAX_CARRY == 0xFFFEF and top[31] == 0
    rng = np.random.default_rng(7)
    for _ in range(64):
        x, y = (int.from_bytes(rng.bytes(32), "little") for _ in range(2))
        assert all(c <= m for c, m in zip(we.mul_carries(x, y)[0], top))


@pytest.mark.parametrize("table", TABLES, ids=IDS)
def test_oracle_trace_is_the_model_and_the_checker_names_the_model_s_rows(oracle, table):
    t = oracle_trace(oracle, table)
    we.check_model(table, t)
    got = host_rows(table, t)
    if table.kind == we.VALID:
        assert got == set(), (table.name, sorted(got))
    assert got == oracle_violated_rows(oracle, table.air_id, t)
    if table.violated is not None:
        assert got == table.violated, (table.name, sorted(got), sorted(table.violated))
    if table.kind == we.FALSE:
        assert got, table.name


def test_the_valid_memory_log_reaches_every_gap_bit(oracle):
    """columns 12 .. 43 (and address_changed): each is non-zero in some row, which random_log and the seeded logs never do
    above bit 19"""
    table = next(t for t in TABLES if t.name == "memory-valid")
    t = oracle_trace(oracle, table)
    assert t[11:44].any(axis=1).all(), np.nonzero(~t[11:44].any(axis=1))[0] + 11
    gaps = {sum(int(t[12 + z, i]) << z for z in range(32)) for i in range(16)}
    assert {0, 0x55555555, 0xAAAAAAAA, 0xFFFFFFFB, 0xFFFFFFFE} <= gaps


def test_the_outside_memory_log_is_rejected_where_the_true_gap_does_not_fit(oracle):
    """what include/bpg.h says of bp_memory_trace outside its ranges: 3 -> 2^32 proves, 2^32 -> p + 5 (stored as 5) and a
    timestamp step of 2^32 + 1 do not, p + 5 -> 2^64 - 1 (stored 5 -> 2^32 - 2, 64-bit difference 2^32 - 7) does"""
    table = next(t for t in TABLES if t.name == "memory-outside")
    assert table.violated == {9, 10}
    t = oracle_trace(oracle, table)
    assert [int(t[1, i]) for i in (8, 10, 12)] == [1 << 32, 5, (1 << 32) - 2]


@pytest.mark.parametrize("table", [t for t in TABLES if t.kind != we.OUTSIDE], ids=[t.name for t in TABLES if t.kind != we.OUTSIDE])
def test_oracle_proof_of_a_table(oracle, table):
    """valid tables: accepted by the oracle's verifier and by bp_stark_verify_air; false logs: rejected by both"""
    cfg = oracle.make_cfg(table.log_n, AIRS[table.air_id].n_cols, num_queries=6, pow_bits=6, air_id=table.air_id)
    proof, ctl, chv = prove(oracle, cfg, oracle_trace(oracle, table))
    assert int(proof[14]) == table.air_id
    if table.kind == we.VALID:
        assert oracle.stark_verify(cfg, proof, ctl, chv, None) == 0 and product_verify(cfg, table.air_id, proof) == 0
    else:
        assert oracle.stark_verify(cfg, proof, ctl, chv, None) != 0 and product_verify(cfg, table.air_id, proof) != 0
