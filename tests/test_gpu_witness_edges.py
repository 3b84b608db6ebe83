"""The seven device witness generators (bp_*_trace, csrc/stark_kernels.hip) at the operand edges include/bpg.h allows:
the tables of tests/witness_edges.py, which tests/test_witness_edges.py proves on the CPU.  Per table: device trace ==
oracle trace bit for bit and == the Python-integer model; the device trace checker names the model's rows; the proof
from the device trace is the oracle's, byte for byte.  Then: seeded and caller-trace proofs are the same bytes for all
seven ids, and the lookup product columns of the narrow tables (AIR 2, 3, 5) against Python integers under five filter
patterns and a zero term, at the heights where aux_suffix_product_kernel changes regime (its launcher uses
min(n, 1024) lanes, at least 64, and a lane owns up to 8 elements per tile: 2^4 fewer elements than lanes -- the
lowest height any entry point accepts, 2^3 is refused --, 2^10 one tile of one element per lane, 2^13 one tile of eight,
2^14 two tiles)."""
import numpy as np
import pytest

import witness_edges as we
from builtin_airs import AIRS, product_verify, prove
from util import P, to_dev, to_host

pytestmark = pytest.mark.gpu
TABLES = we.all_tables()
IDS = [t.name for t in TABLES]
PROVEN = [t for t in TABLES if t.kind != we.OUTSIDE]
_CACHE = {}


def device_trace(bpg, table):
    """the device generator's trace of the table (device tensor), made once"""
    if table.name not in _CACHE:
        _CACHE[table.name] = bpg.ops.air_trace(table.air_id, table.log_n, inputs=to_dev(table.inputs))
    return _CACHE[table.name]


def oracle_trace(oracle, table):
    return oracle.air_trace(table.air_id, table.log_n, inputs=table.inputs)


# ------------------------------------------------------------------------------------------------ a. the trace


@pytest.mark.parametrize("table", TABLES, ids=IDS)
def test_device_trace_is_the_oracle_s_and_the_model_s(bpg, oracle, table):
    got = to_host(device_trace(bpg, table))
    want = oracle_trace(oracle, table)
    assert got.shape == want.shape
    assert we.first_difference(table, got, want) is None, "%s: %s" % (table.name, we.first_difference(table, got, want))
    we.check_model(table, got)            # the model on the device's own words: a mistake shared with the oracle shows


# ------------------------------------------------------------------------------------------------ b. the checker


@pytest.mark.parametrize("table", TABLES, ids=IDS)
def test_device_checker_on_the_device_trace(bpg, table):
    trace = device_trace(bpg, table)
    n = 1 << table.log_n
    res = bpg.ops.check_air_trace(table.air_id, trace, max_rows=n)
    assert res.n_violated_rows == len(res.rows)
    rows = set(res.rows)
    if table.kind == we.VALID:
        assert rows == set(), (table.name, sorted(rows))
    elif table.kind == we.FALSE:
        assert rows == table.violated and rows, (table.name, sorted(rows), sorted(table.violated))
    else:                                  # outside: agreement with the host checker on the same words, nothing more
        host = bpg.ops.check_air_trace_host(table.air_id, to_host(trace), max_rows=n)
        assert rows == set(host.rows) and res.n_violated_rows == host.n_violated_rows, (table.name, sorted(rows), host.rows)


# ------------------------------------------------------------------------------------------------ c. the proof


@pytest.mark.parametrize("table", PROVEN, ids=[t.name for t in PROVEN])
def test_proof_from_the_device_trace_is_the_oracle_s(bpg, oracle, table):
    """valid tables: bytes equal, both verifiers accept, one flipped bit is rejected; false logs: the proof is produced
    (the prover does not judge its witness), equals the oracle's, and both verifiers reject it"""
    n_cols = AIRS[table.air_id].n_cols
    cfg = oracle.make_cfg(table.log_n, n_cols, num_queries=6, pow_bits=6, air_id=table.air_id)
    want, ctl, chv = prove(oracle, cfg, oracle_trace(oracle, table))
    pc = bpg.ops.stark_cfg(table.log_n, n_cols, num_queries=6, pow_bits=6)
    got = bpg.ops.stark_prove_trace(table.air_id, pc, device_trace(bpg, table))
    assert got.shape == want.shape and int(got[14]) == table.air_id
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: first mismatch at word %d of %d" % (table.name, bad[0], want.size)
    if table.kind == we.VALID:
        assert oracle.stark_verify(cfg, got, ctl, chv, None) == 0
        assert product_verify(pc, table.air_id, got) == 0
        flipped = got.copy()
        flipped[got.size // 2] ^= np.uint64(1 << 21)
        assert product_verify(pc, table.air_id, flipped) != 0
    else:
        assert oracle.stark_verify(cfg, got, ctl, chv, None) != 0
        assert product_verify(pc, table.air_id, got) != 0


# ------------------------------------------------------------------------------------------------ d. seeded == caller's


@pytest.mark.parametrize("loaded", [0, 1], ids=["spread", "one-pass"])
@pytest.mark.parametrize("air_id", [1, 2, 3, 4, 5, 6, 7])
def test_seeded_and_caller_trace_proofs_are_the_same_bytes(bpg, air_id, loaded):
    """what include/bpg.h promises of bp_stark_prove_trace(built-in id, bp_*_trace(seed)); 2^5 rows (AIR 1: one
    permutation and a part of the next)"""
    seed = 0x5EED0E00 + air_id
    pc = bpg.ops.stark_cfg(5, AIRS[air_id].n_cols, num_queries=6, pow_bits=6)
    trace = bpg.ops.air_trace(air_id, 5, seed=seed)
    with bpg.ops.tuned(assume_loaded=loaded):
        want = bpg.ops.stark_prove_air(air_id, pc, seed)
        got = bpg.ops.stark_prove_trace(air_id, pc, trace)
    bad = np.nonzero(got != want)[0] if got.shape == want.shape else [-1]
    assert len(bad) == 0, "AIR %d: first mismatch at word %d of %d" % (air_id, bad[0], want.size)
    assert product_verify(pc, air_id, got) == 0


# ------------------------------------------------------------------------------------------------ e. lookup products

CTL = [0x0123456789ABCDEF % P, 0xFEDCBA9876543210 % P, 0x0F1E2D3C4B5A6978 % P, 0x8877665544332211 % P]  # beta0 gamma0 beta1 gamma1


def _filters(n):
    i = np.arange(n)
    return [("none", np.zeros(n, dtype=np.int64)), ("all", np.ones(n, dtype=np.int64)), ("alternating", (i % 2 == 0).astype(np.int64)),
            ("first", (i == 0).astype(np.int64)), ("last", (i == n - 1).astype(np.int64))]


def _set_filter(air_id, trace, f):
    """AIR 2 / 3: the filter is the trace column g; AIR 5: "the row has a length", the sum of its 32 length flags"""
    import torch
    f = torch.from_numpy(f).cuda()
    if air_id == 5:
        trace[1:33] = 0
        rows = torch.arange(trace.shape[1], device="cuda")
        trace[1 + rows % 32, rows] = f
    else:
        trace[{2: 523, 3: 44}[air_id]] = f
    return trace


def test_no_entry_reaches_the_product_kernel_below_sixteen_rows(bpg):
    """why the "fewer elements than lanes" regime is tested at 2^4 (16 rows, 64 lanes) and not at 2^3"""
    import torch
    from proof_protocol_decoder_amd._lib import BpgError
    with pytest.raises(BpgError, match="log_n out of range"):
        bpg.ops.memory_trace(3, seed=1)
    with pytest.raises(BpgError, match="log_n out of range"):
        bpg.ops.debug_air_aux(3, torch.zeros((45, 8), dtype=torch.int64, device="cuda"), CTL)


@pytest.mark.parametrize("log_n", [4, 10, 13, 14])
@pytest.mark.parametrize("air_id", [2, 3, 5])
def test_lookup_products_with_a_filter_set_against_python_integers(bpg, air_id, log_n):
    n = 1 << log_n
    if log_n == 4:                         # the first sixteen rows of the edge table
        table = next(t for t in TABLES if t.air_id == air_id and t.kind == we.VALID)
        trace = bpg.ops.air_trace(air_id, 4, inputs=to_dev(table.inputs[:16]))
    else:
        trace = bpg.ops.air_trace(air_id, log_n, seed=0xA0C5 + 16 * air_id + log_n)
    tup, _ = we.lookup_tuple(air_id, to_host(trace))
    v = [we.compress(tup, CTL[0]), we.compress(tup, CTL[2])]   # the compressed tuple does not depend on the filter
    assert len(set(v[0])) > 1
    for name, f in _filters(n):
        t = _set_filter(air_id, trace.clone(), f)
        filt = [int(x) for x in f]
        as_read = t[1:33].sum(dim=0) if air_id == 5 else t[{2: 523, 3: 44}[air_id]]
        assert as_read.cpu().tolist() == filt, name
        got = to_host(bpg.ops.debug_air_aux(air_id, t, CTL))
        assert got.shape == (2, n)
        for c in range(2):
            want = we.suffix_products(filt, v[c], CTL[2 * c + 1])
            bad = [i for i in range(n) if int(got[c, i]) != want[i]]
            assert not bad, "AIR %d, 2^%d rows, filter %s, z_%d: first mismatch at row %d" % (air_id, log_n, name, c, bad[0])
        if name == "none":
            assert (got == 1).all()
    # gamma_0 chosen so that the term of one filtered row is zero: z_0 is zero at and before it (across tiles: the row is
    # in the last quarter), the rows after it and all of z_1 are what they were
    r0 = n // 2 + n // 4
    name, f = _filters(n)[2]
    assert f[r0] == 1
    ctl = list(CTL)
    ctl[1] = (-v[0][r0]) % P
    t = _set_filter(air_id, trace.clone(), f)
    filt = [int(x) for x in f]
    got = to_host(bpg.ops.debug_air_aux(air_id, t, ctl))
    want0, want1 = we.suffix_products(filt, v[0], ctl[1]), we.suffix_products(filt, v[1], ctl[3])
    assert not any(want0[:r0 + 1]) and all(want0[r0 + 1:])
    assert not got[0, :r0 + 1].any(), "zero does not reach row %d" % int(np.nonzero(got[0, :r0 + 1])[0][-1])
    assert [int(x) for x in got[0, r0 + 1:]] == want0[r0 + 1:]
    assert [int(x) for x in got[1]] == want1
