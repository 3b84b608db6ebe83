"""The AIR trace checker on the CPU (bp_air_check_trace_host: csrc/air_check.cpp over air.hpp's evaluators) against
oracle-made traces: valid witnesses report nothing, a corrupted cell is named at its row with a constraint of the family
the AIR's own tests break, and the rows (and, for the AIRs of at most ~600 constraints, the constraint values) agree
with an independent evaluation by the oracle.  Also: argument errors, and the device source's register / hazard rules
(the rules tests/test_build.py applies to its three kernel sources).  GPU side: tests/test_gpu_air_check.py."""
import re

import numpy as np
import pytest

from air_check_util import P, oracle_constraint_values, oracle_violated_rows, selectors
from builtin_airs import AIRS, checker_breaks, memory

LOG_N = 6


def ops():
    import proof_protocol_decoder_amd as pkg
    pkg.lib()
    return pkg.ops


def seeded(oracle, air_id, log_n=LOG_N, seed=0xC0DE):
    return oracle.air_trace(air_id, log_n, seed=seed)


def family_name(air_id, family):
    """describe()'s family list of each AIR starts with its own families, in the order of their names"""
    return "%s%d" % (AIRS[air_id].prefix, family)


@pytest.mark.parametrize("air_id", sorted(AIRS))
def test_seeded_traces_satisfy_their_air(oracle, air_id):
    for seed in (1, 0xC0DE):
        r = ops().check_air_trace_host(air_id, seeded(oracle, air_id, seed=seed))
        assert r.ok and r.n_violated_rows == 0 and r.rows == [] and r.violations == [], r


def test_synthetic_trace_with_constants_satisfies_its_air(oracle):
    cfg = oracle.make_cfg(LOG_N, 32, n_const=3)
    consts = oracle.synth_constants(9, LOG_N, 3)
    t = oracle.synth_trace(0x51, cfg, consts)
    o = ops()
    assert o.check_air_trace_host(0, t, consts=consts).ok
    bad = t.copy()
    bad[4 * 2 + 2, 10] ^= np.uint64(1)          # c of group 2 at row 10: c - a b - q a (index 6) and d' - (a b c)^e - b (7)
    r = o.check_air_trace_host(0, bad, consts=consts)
    assert r.rows == [10] and [(v.row, v.constraint, v.family, v.kind) for v in r.violations] == [(10, 6, 0, 0), (10, 7, 1, 1)]
    bad = t.copy()
    bad[4 * 1 + 3, 0] ^= np.uint64(1)           # d of group 1 in row 0: first-row d - a - b (index 5), and the transition
    r = o.check_air_trace_host(0, bad, consts=consts)   # into row 0 from the last row does not apply
    assert r.rows == [0] and {(v.constraint, v.kind) for v in r.violations} == {(5, 2)}
    bad = t.copy()
    bad[4 * 1 + 3, 20] ^= np.uint64(1)          # d of group 1 in row 20: the transition from row 19 (index 4)
    r = o.check_air_trace_host(0, bad, consts=consts)
    assert r.rows == [19] and {(v.constraint, v.family, v.kind) for v in r.violations} == {(4, 1, 1)}


# (air, column, row, value or None for "xor 1", the families any of which may be named): the cell breaks of
# tests/builtin_airs.py whose target is the AIR itself (the lookup filters' constraints are not the AIR's)
BREAKS = checker_breaks()


@pytest.mark.parametrize("air_id,col,row,val,fams", BREAKS, ids=["%d-%s@%d" % (b[0], b[4].replace(" ", "/"), b[2]) for b in BREAKS])
def test_a_corrupted_cell_is_named_at_its_row_with_its_family(oracle, air_id, col, row, val, fams):
    t = seeded(oracle, air_id)
    t[col, row] = np.uint64(val) if val is not None else t[col, row] ^ np.uint64(1)
    r = ops().check_air_trace_host(air_id, t, max_rows=64)
    assert r.n_violated_rows >= 1 and set(r.rows) <= {row - 1, row}, r
    assert {v.row for v in r.violations} == set(r.rows)
    named = {family_name(air_id, v.family) for v in r.violations}
    assert named & set(fams.split()), (named, fams)
    d = ops().air_describe(air_id)
    for v in r.violations:   # transition constraints are reported at the row before the changed "next" row
        f = d.families[v.family]
        assert f.first_index <= v.constraint < f.first_index + f.count and v.kind == f.kind
        assert v.row == row or v.kind == 1
        assert 0 < v.value < P


def test_a_stale_memory_read_is_named_at_the_row_before(oracle):
    log = memory.random_log(64, 11, n_addr=6)
    r0 = next(i for i in range(1, 64) if log[i, 0] == 1 and log[i, 1] == log[i - 1, 1])
    log[r0, 3 + 2] ^= np.uint64(5)
    r = ops().check_air_trace_host(3, oracle.memory_trace(6, inputs=log))
    assert r.rows == [r0 - 1] and {family_name(3, v.family) for v in r.violations} == {"M5"}


def _corrupt(t, k, rng):
    rows = sorted(rng.choice(t.shape[1], size=k, replace=False))
    for i in rows:
        c = int(rng.integers(0, t.shape[0]))
        t[c, i] = (int(t[c, i]) + 1 + int(rng.integers(0, 3))) % P
    return rows


@pytest.mark.parametrize("air_id", sorted(AIRS))
def test_rows_agree_with_the_oracle(oracle, air_id):
    """The rows the host entry reports are exactly those whose oracle fold (orc_*_constraints_base with the trace
    domain's selectors) is non-zero; for the AIRs of at most ~600 constraints the values too, constraint by constraint."""
    rng = np.random.default_rng(air_id)
    o = ops()
    d = o.air_describe(air_id)
    T = d.n_air_constraints
    for trial in range(2):
        t = seeded(oracle, air_id, seed=0x100 + trial)
        _corrupt(t, 3, rng)
        r = o.check_air_trace_host(air_id, t, max_rows=64, max_viol=1 << 16)
        assert set(r.rows) == oracle_violated_rows(oracle, air_id, t) and r.n_violated_rows == len(r.rows)
        assert r.n_violations == len(r.violations)
        if T > 600:
            continue
        for i in r.rows:
            want = oracle_constraint_values(oracle, air_id, t, i, T)
            got = {v.constraint: v for v in r.violations if v.row == i}
            assert {idx for idx, c in enumerate(want) if c} == set(got)
            z_last, l_first, l_last = selectors(i, t.shape[1].bit_length() - 1)
            for idx, v in got.items():
                sel = {0: 1, 1: z_last, 2: l_first, 3: l_last}[v.kind]
                assert want[idx] == v.value * sel % P, (i, idx)


def test_max_rows_truncates_and_a_strided_trace_is_read_in_place(oracle):
    t = seeded(oracle, 3, log_n=8)
    for i in (5, 77, 130, 200):
        t[0, i] = 2                                  # is_read not a bit (M0 at row i; the read rule may break at i - 1)
    o = ops()
    full = o.check_air_trace_host(3, t, max_rows=64)
    assert {5, 77, 130, 200} <= set(full.rows) <= {4, 5, 76, 77, 129, 130, 199, 200}
    assert full.n_violated_rows == len(full.rows) and full.rows == sorted(full.rows)
    r = o.check_air_trace_host(3, t, max_rows=2)
    assert r.n_violated_rows == full.n_violated_rows and r.rows == full.rows[:2]
    assert {v.row for v in r.violations} == set(full.rows[:2])
    wide = np.zeros((t.shape[0], 300), dtype=np.uint64)
    wide[:, :256] = t
    wide[:, 256:] = 12345                            # past the trace: never read
    r2 = o.check_air_trace_host(3, wide[:, :256], max_rows=64)
    assert r2.rows == full.rows and [(v.row, v.constraint, v.value) for v in r2.violations] == \
        [(v.row, v.constraint, v.value) for v in full.violations]
    r3 = o.check_air_trace_host(3, t, max_rows=64, max_viol=1)
    assert len(r3.violations) == 1 and r3.n_violations == full.n_violations > 1


def test_argument_errors_are_refused(oracle):
    import ctypes as C
    from proof_protocol_decoder_amd._lib import AirViolation, BpgError, StarkCfg
    o = ops()
    t = seeded(oracle, 3)
    with pytest.raises(BpgError, match="INVALID_INPUT"):
        o.check_air_trace_host(3, t[:44])                         # memory is 45 columns wide
    with pytest.raises(BpgError, match="INVALID_INPUT"):
        o.check_air_trace_host(3, np.ascontiguousarray(t[:, :8]))  # 2^3 rows: log_n out of range
    with pytest.raises(BpgError, match="INVALID_INPUT"):
        o.check_air_trace_host(9, t)                               # no AIR 9
    with pytest.raises(BpgError, match="INVALID_INPUT"):
        o.check_air_trace_host(8, np.zeros((135, 64), dtype=np.uint64))  # AIR 8 without constants / public inputs
    L = o.lib()
    cfg = o.stark_cfg(LOG_N, 45)
    n_rows, n_viol = C.c_uint64(), C.c_uint32()
    rows, viol = (C.c_uint32 * 4)(), (AirViolation * 4)()
    assert L.bp_air_check_trace_host(3, C.byref(cfg), t.ctypes.data, 63, None, None, 4, C.byref(n_rows), rows, viol, 4,
                                     C.byref(n_viol)) == -2           # stride shorter than the trace
    assert L.bp_air_check_trace_host(3, C.byref(cfg), None, 64, None, None, 4, C.byref(n_rows), rows, viol, 4,
                                     C.byref(n_viol)) == -2
    assert L.bp_air_check_trace_host(3, C.byref(cfg), t.ctypes.data, 64, None, None, 4, C.byref(n_rows), None, viol, 4,
                                     C.byref(n_viol)) == -2           # max_rows > 0 without room for them
    assert L.bp_air_check_trace_host(3, None, t.ctypes.data, 64, None, None, 4, C.byref(n_rows), rows, viol, 4,
                                     C.byref(n_viol)) == -2
    bad_rate = StarkCfg(LOG_N, 45, 0, 1, 2, 4, 84, 16, 4, 5)
    assert L.bp_air_check_trace_host(3, C.byref(bad_rate), t.ctypes.data, 64, None, None, 4, C.byref(n_rows), rows, viol,
                                     4, C.byref(n_viol)) == -2
    assert L.bp_air_check_trace(3, C.byref(cfg), None, 64, None, None, 4, C.byref(n_rows), rows, viol, 4,
                                C.byref(n_viol), None) == -2          # (refused before any device call)


# ---- the device source under the rules tests/test_build.py applies to its three kernel sources


def test_air_check_kernels_have_no_scratch_and_spill_only_arguments(tmp_path):
    from test_build import device_assembly
    asm = device_assembly("air_check.hip", tmp_path)
    name, seen = None, 0
    for line in asm.splitlines():
        m = re.match(r"\s+\.name:\s+(\S+)", line)
        if m:
            name = m.group(1)
            seen += "air_check" in name
        m = re.match(r"\s+\.private_segment_fixed_size:\s+(\d+)", line)
        if m:
            assert int(m.group(1)) == 0, (name, "scratch")
        m = re.match(r"\s+\.sgpr_spill_count:\s+(\d+)", line)
        if m:
            assert int(m.group(1)) <= (40 if "air_check_kernel" in name else 0), (name, int(m.group(1)))
    assert seen >= 13   # nine AIRs, the Poseidon-gate pass, the reduction, the alpha table, the row gather


def test_air_check_kernels_have_no_carry_mask_hazard(tmp_path):
    from test_build import device_assembly, scan_carry_mask_hazards
    bad, n = scan_carry_mask_hazards(device_assembly("air_check.hip", tmp_path))
    assert n > 1000 and not bad, bad[:10]


def test_air_check_kernels_have_no_dpp_read_of_a_fresh_asm_result(tmp_path):
    """test_build.test_no_dpp_reads_a_fresh_asm_result's rule on air_check.hip"""
    from test_build import _vregs, device_assembly
    in_asm, recent, bad = False, [], []
    for ln, line in enumerate(device_assembly("air_check.hip", tmp_path).splitlines(), 1):
        t = line.strip()
        if t.startswith(";") and "ASMSTART" in t:
            in_asm = True
            continue
        if t.startswith(";") and "ASMEND" in t:
            in_asm = False
            continue
        if not t or t.startswith((";", ".", "//")) or t.endswith(":"):
            continue
        op = t.split()[0]
        if not re.match(r"[sv]_|ds_|global_|buffer_|flat_|scratch_", op):
            continue
        operands = [x.strip() for x in t[len(op):].split(";")[0].replace(" quad_perm", ", quad_perm").split(",")]
        states = int(operands[0], 0) + 1 if op == "s_nop" else 1
        is_swap = op.startswith("v_permlane") and "swap" in op
        if "_dpp" in op or "quad_perm" in t or "row_" in t or op.startswith("v_permlane"):
            srcs = set()
            for o in (operands if is_swap else operands[1:]):
                srcs |= _vregs(o.split()[0] if o else o)
            bad += [(ln, t) for age, regs in recent if age < 2 and regs & srcs]
        recent = [(age + states, regs) for age, regs in recent if age + states < 2]
        if in_asm and op.startswith("v_") and operands:
            recent.append((0, _vregs(operands[0]) | (_vregs(operands[1]) if is_swap and len(operands) > 1 else set())))
    assert not bad, bad


def test_shapes_the_entry_cannot_read_are_refused_before_the_call(oracle):
    o = ops()
    with pytest.raises(ValueError, match="2\\^log_n rows"):
        o.check_air_trace_host(3, np.zeros((45, 100), dtype=np.uint64))
    with pytest.raises(ValueError, match="constants must be"):
        o.check_air_trace_host(8, np.zeros((135, 64), dtype=np.uint64), consts=np.zeros((85, 32), dtype=np.uint64), pub=[0] * 4)
    with pytest.raises(ValueError, match="four public inputs"):
        o.check_air_trace_host(8, np.zeros((135, 64), dtype=np.uint64), consts=np.zeros((85, 64), dtype=np.uint64), pub=[0] * 3)
