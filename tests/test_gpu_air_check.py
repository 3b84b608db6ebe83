"""The AIR trace checker on the GPU (bp_air_check_trace: csrc/air_check.hip marks the rows, csrc/air_check.cpp names the
constraints): device witnesses satisfy their AIRs at small and at reference heights; on corrupted traces the device's
row set is the host entry's (bp_air_check_trace_host on the downloaded trace) and the oracle's; rows 0 and n - 1,
max_rows and a strided trace; AIR 8 with its constants and public inputs.  CPU side: tests/test_air_check.py."""
import ctypes as C

import numpy as np
import pytest

from air_check_util import P, oracle_violated_rows
from builtin_airs import AIRS, memory
from util import to_dev, to_host

pytestmark = pytest.mark.gpu

# one reference height per table: Keccak-f 2^14, memory 2^17, the others at upstream's lower bounds (constants.rs;
# arithmetic_mul is the arithmetic table's other half)
REF_LOG_N = {1: 14, 2: 12, 3: 17, 4: 16, 5: 9, 6: 9, 7: 16}


def dev_trace(bpg, air_id, log_n, seed):
    return bpg.ops.air_trace(air_id, log_n, seed=seed)


def corrupt(t, k, rng):
    """k cells in k distinct rows changed on the device tensor; returns the rows"""
    rows = sorted(int(x) for x in rng.choice(t.shape[1], size=k, replace=False))
    for i in rows:
        c = int(rng.integers(0, t.shape[0]))
        v = int(t[c, i].item()) & (2 ** 64 - 1)
        nv = (v + 1 + int(rng.integers(0, 3))) % P
        t[c, i] = nv - (1 << 64) if nv >= 1 << 63 else nv
    return rows


@pytest.mark.parametrize("air_id", sorted(AIRS))
def test_device_witnesses_satisfy_their_air(bpg, air_id):
    for log_n in (6, REF_LOG_N[air_id]):
        r = bpg.ops.check_air_trace(air_id, dev_trace(bpg, air_id, log_n, 0xA1 + log_n))
        assert r.ok and r.rows == [] and r.violations == [], (log_n, r)


def test_given_memory_log_satisfies_its_air(bpg):
    log = memory.random_log(256, 5)
    t = bpg.ops.memory_trace(8, inputs=to_dev(log))
    assert bpg.ops.check_air_trace(3, t).ok
    log[40, 3] ^= np.uint64(1)   # a value limb of one operation: whatever it breaks, host and device see the same rows
    bad = bpg.ops.memory_trace(8, inputs=to_dev(log))
    r = bpg.ops.check_air_trace(3, bad, max_rows=256)
    assert r.rows == bpg.ops.check_air_trace_host(3, to_host(bad), max_rows=256).rows


@pytest.mark.parametrize("air_id", sorted(AIRS))
def test_device_rows_equal_the_host_entry_and_the_oracle(bpg, oracle, air_id):
    log_n = 6 + (air_id % 5)     # 2^6 .. 2^10
    rng = np.random.default_rng(0x700 + air_id)
    t = dev_trace(bpg, air_id, log_n, 0xB0 + air_id)
    corrupt(t, 4, rng)
    n = 1 << log_n
    r = bpg.ops.check_air_trace(air_id, t, max_rows=n)
    h = to_host(t)
    hr = bpg.ops.check_air_trace_host(air_id, h, max_rows=n)
    assert r.n_violated_rows == hr.n_violated_rows == len(r.rows) > 0
    assert r.rows == hr.rows
    assert set(r.rows) == oracle_violated_rows(oracle, air_id, h)
    key = lambda v: (v.row, v.constraint, v.family, v.kind, v.value)
    assert [key(v) for v in r.violations] == [key(v) for v in hr.violations]


@pytest.mark.parametrize("air_id", [1, 3])
def test_large_heights_give_the_host_entrys_rows(bpg, air_id):
    rng = np.random.default_rng(0x900 + air_id)
    t = dev_trace(bpg, air_id, REF_LOG_N[air_id], 0xC0 + air_id)
    corrupt(t, 6, rng)
    r = bpg.ops.check_air_trace(air_id, t, max_rows=64)
    hr = bpg.ops.check_air_trace_host(air_id, to_host(t), max_rows=64)
    assert r.n_violated_rows == hr.n_violated_rows > 0 and r.rows == hr.rows


def test_first_and_last_rows_max_rows_and_a_strided_trace(bpg):
    import torch
    log_n = 10
    n = 1 << log_n
    t = bpg.ops.memory_trace(log_n, seed=0x5E)
    t[0, n - 1] = 2             # is_read of the last row: M0 there (its transition into row 0 does not apply)
    t[3 + 1, 0] = 77            # a value limb of row 0: the first-row family M7 if row 0 reads, else only the row before's rules
    t[0, 0] = 1                 # make row 0 a read: M7 (first access reads zero) at row 0
    r = bpg.ops.check_air_trace(3, t, max_rows=n)
    hr = bpg.ops.check_air_trace_host(3, to_host(t), max_rows=n)
    assert r.rows == hr.rows and 0 in r.rows and n - 1 in r.rows
    fams = {(v.row, v.family) for v in r.violations}
    assert (0, 7) in fams and (n - 1, 0) in fams
    assert not any(v.kind == 1 and v.row == n - 1 for v in r.violations)   # no transition out of the last row
    d = bpg.ops.check_air_trace(3, t, max_rows=1)
    assert d.n_violated_rows == r.n_violated_rows and d.rows == r.rows[:1] and {v.row for v in d.violations} == {r.rows[0]}
    wide = torch.full((t.shape[0], n + 320), 12345, dtype=torch.int64, device="cuda")
    wide[:, :n] = t
    w = bpg.ops.check_air_trace(3, wide[:, :n], max_rows=n)
    assert w.rows == r.rows and [(v.row, v.constraint, v.value) for v in w.violations] == [(v.row, v.constraint, v.value) for v in r.violations]


def test_keccak_f_rows_zero_and_last(bpg):
    t = bpg.ops.keccak_trace(8, seed=0x3)
    n = 256
    t[0, 0] = 0                 # the step flag of row 0: F0 (first row: step 0 is set) at row 0
    t[24 + 3, n - 1] = 5        # an input limb of the last row
    r = bpg.ops.check_air_trace(1, t, max_rows=n)
    assert r.rows == bpg.ops.check_air_trace_host(1, to_host(t), max_rows=n).rows
    assert (0, 0) in {(v.row, v.family) for v in r.violations} and n - 1 in r.rows


def test_air8_with_its_constants_and_public_inputs(bpg, oracle):
    import torch
    from test_gpu_plonk_air import Layout, dev_constants
    log_n = 7
    k = dev_constants(bpg, log_n, 0xC0DE08, pi_len=9)
    pi = [int(x) for x in np.random.default_rng(8).integers(0, P, size=9, dtype=np.uint64)]
    t = torch.empty((135, 1 << log_n), dtype=torch.int64, device="cuda")
    L = bpg.lib()
    lay = Layout(len(pi), 0, 0, 0, 0)
    bpg._lib.check(L.bp_plonk_trace(C.c_void_p(k.data_ptr()), C.c_uint64(0x5EED08), (C.c_uint64 * len(pi))(*pi), C.byref(lay),
                                    None, log_n, C.c_void_p(t.data_ptr()), None))
    pub = [int(x) for x in oracle.hash_no_pad(np.array(pi, dtype=np.uint64))]
    assert [int(x) & (2 ** 64 - 1) for x in t[:4, 0].tolist()] == pub
    assert bpg.ops.check_air_trace(8, t, consts=k, pub=pub).ok
    wrong = list(pub)
    wrong[2] = (wrong[2] + 1) % P
    r = bpg.ops.check_air_trace(8, t, consts=k, pub=wrong)       # the public-input row: G3 at row 0
    assert r.rows == [0] and {(v.family, v.kind, v.constraint) for v in r.violations} == {(3, 2, 86 + 2)}
    for col, row, fam in ((3, 20, 0), (24 + 5, 4, 4), (130, 5, 5)):   # an arithmetic gate's d, a Poseidon round wire, the swap bit
        bad = t.clone()
        v = (int(bad[col, row].item()) % (1 << 64) + 2) % P        # stays canonical
        bad[col, row] = v - (1 << 64) if v >= 1 << 63 else v
        r = bpg.ops.check_air_trace(8, bad, consts=k, pub=pub)
        hr = bpg.ops.check_air_trace_host(8, to_host(bad), consts=to_host(k), pub=pub)
        assert r.rows == hr.rows == [row], (col, row, r)
        assert fam in {v.family for v in r.violations}
        assert [(v.constraint, v.value) for v in r.violations] == [(v.constraint, v.value) for v in hr.violations]


def test_argument_errors_are_refused_on_the_device(bpg):
    t = bpg.ops.memory_trace(6, seed=1)
    with pytest.raises(Exception, match="INVALID_INPUT"):
        bpg.ops.check_air_trace(3, t[:44].contiguous())
    with pytest.raises(Exception, match="INVALID_INPUT"):
        bpg.ops.check_air_trace(8, bpg.ops.memory_trace(6, seed=1).repeat(3, 1)[:135].contiguous())   # no constants
