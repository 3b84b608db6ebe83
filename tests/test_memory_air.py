"""AIR 3 (a memory log sorted by address, then timestamp) on the CPU: the oracle's witness against a Python model of a
memory, its constraint list against the witness, and its proofs against the PRODUCT's CPU verifier (csrc/air.hpp over
the extension field) -- two independent statements of the same 60 constraints.  The record of the AIR and the shared
test bodies: tests/builtin_airs.py; GPU side: tests/test_gpu_memory_air.py."""
import numpy as np
import pytest

import builtin_airs as ba
from builtin_airs import P, memory as air

COL_READ, COL_CHG, N_COLS = air.COL_READ, air.COL_CHG, air.n_cols


def test_traces_are_consistent_memories(oracle):
    log = air.random_log(64, 3)
    t = oracle.memory_trace(6, inputs=log)
    assert t.shape == (N_COLS, 64) and (t < np.uint64(P)).all()
    assert (t[:COL_CHG].T == log).all()
    air.check_trace_is_a_memory(t)
    s1 = oracle.memory_trace(8, seed=0x77)
    air.check_trace_is_a_memory(s1)
    assert (oracle.memory_trace(8, seed=0x77) == s1).all() and (oracle.memory_trace(8, seed=0x78) != s1).any()
    assert 0 < int(s1[COL_READ].sum()) < 256 and int(s1[COL_CHG].sum()) == 63   # four operations per address


@pytest.mark.parametrize("log_n,seeded", [(5, True), (7, False), (9, True)])
def test_oracle_proof_is_accepted_by_both_verifiers_and_tampering_is_not(oracle, log_n, seeded):
    trace = oracle.memory_trace(log_n, seed=0xFACE + log_n) if seeded else oracle.memory_trace(log_n, inputs=air.random_log(1 << log_n, log_n))
    ba.check_proof_is_accepted_and_tampering_is_not(oracle, air, log_n, trace)


def _broken_logs():
    """Logs that are NOT a memory: each breaks one thing the AIR exists to enforce."""
    base = air.random_log(64, 11, n_addr=6)
    out = []
    b = base.copy()                       # a read returns something else than what was written
    r = next(i for i in range(1, 64) if b[i, 0] == 1 and b[i, 1] == b[i - 1, 1])
    b[r, 3 + 2] ^= np.uint64(5)
    out.append(("M5 stale read", b))
    b = base.copy()                       # the first access of an address is a read of non-zero memory
    r = next(i for i in range(1, 64) if b[i, 1] != b[i - 1, 1])
    b[r, 0], b[r, 3] = 1, 7
    out.append(("M6 first read not zero", b))
    b = base.copy()                       # timestamps go backwards inside an address
    r = next(i for i in range(1, 64) if b[i, 1] == b[i - 1, 1])
    b[r, 2] = b[r - 1, 2] - np.uint64(1) if b[r, 0] == 0 else b[r - 1, 2]
    if b[r, 0] == 1:
        b[r, 0] = 0
    out.append(("M4 time does not advance", b))
    b = base.copy()                       # addresses not sorted
    r = next(i for i in range(1, 64) if b[i, 1] != b[i - 1, 1])
    b[r:, 1] = b[r - 1, 1] - np.uint64(1)
    b[r:, 0] = 0
    out.append(("M4 addresses go down", b))
    b = base.copy()
    b[0, 0], b[0, 3 + 7] = 1, 9           # the very first row reads a non-zero value
    out.append(("M7 first row", b))
    return out


@pytest.mark.parametrize("what,log", _broken_logs(), ids=[w for w, _ in _broken_logs()])
def test_a_log_that_is_not_a_memory_yields_a_rejected_proof(oracle, what, log):
    """The witness generator follows the log it is given; the verifier must refuse what is not a memory."""
    cfg = ba.small_cfg(oracle, air, 6)
    trace = oracle.memory_trace(6, inputs=log)
    proof, ctl, chv = ba.prove(oracle, cfg, trace)
    assert oracle.stark_verify(cfg, proof, ctl, chv, None) != 0
    assert ba.product_verify(cfg, 3, proof) != 0


@pytest.mark.parametrize("brk", air.breaks, ids=[b.label for b in air.breaks])
def test_a_witness_cell_out_of_range_is_rejected(oracle, brk):
    ba.check_break_yields_a_rejected_proof(oracle, air, brk)


def test_air_registry_describes_the_memory_air():
    ba.check_registry_describes(air)
