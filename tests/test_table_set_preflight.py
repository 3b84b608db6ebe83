"""The pre-flight of table sets, the part that needs no GPU: the Python model of bp_check_table_set's link report
(tests/table_set_model.py) against a brute-force restatement of the header's definitions; the statement's refusals
through the new entry, before a device is touched; and the project's build rules on csrc/set_check.hip.  GPU side:
tests/test_gpu_table_set_preflight.py."""
import re

import numpy as np
import pytest

import air_program_cases as cases
import air_program_port_cases as pc
import table_set_model as model
from air_program_cases import P
from proof_protocol_decoder_amd._lib import BpgError


@pytest.fixture(scope="module")
def bpg():
    """the package with its library loaded: nothing here touches a device"""
    import proof_protocol_decoder_amd as pkg
    pkg.lib()
    return pkg


# ---------------------------------------------------------------------------------------------- 1. the model


def brute_force(ends, wants_bit):
    """the header's sentences one by one, quadratic: per tuple value the two sums, then the minima"""
    n_looking = len(ends) - 1
    kept = [(m, i, f, model.strip(t)) for m, rows in enumerate(ends) for i, (f, t) in enumerate(rows) if f != 0]
    values = []
    for _, _, _, v in kept:
        if v not in values:
            values.append(v)
    off = []
    for v in values:
        looking = sum(f for m, _, f, w in kept if w == v and m < n_looking)
        looked = sum(f for m, _, f, w in kept if w == v and m == n_looking)
        if (looking - looked) % P:
            off.append(v)
    looking_rows = sorted((m, i) for m, i, _, v in kept if m < n_looking and v in off)
    looked_rows = sorted(i for m, i, _, v in kept if m == n_looking and v in off)
    bad = sorted((m, i, f) for m, rows in enumerate(ends) for i, (f, _) in enumerate(rows) if wants_bit[m] and f not in (0, 1))
    return {"holds": not off and not bad, "n_looking": sum(m < n_looking for m, _, _, _ in kept),
            "n_looked": sum(m == n_looking for m, _, _, _ in kept), "n_unbalanced": len(off),
            "first_looking_end": looking_rows[0][0] if looking_rows else -1, "first_looking_row": looking_rows[0][1] if looking_rows else -1,
            "first_looked_row": looked_rows[0] if looked_rows else -1,
            "bad_filter_end": bad[0][0] if bad else -1, "bad_filter_row": bad[0][1] if bad else -1, "bad_filter_value": bad[0][2] if bad else 0}


def tiny_link(seed):
    """1 .. 3 looking ends and a looked end of 4 .. 12 rows, tuples of 1 .. 3 elements from {0, 1, 2} (so trailing zeros,
    duplicates and partial cancellations abound), filters mostly bits, some multiplicities, p - 1 and 2 among them"""
    rng = np.random.default_rng(seed)
    ends, bits = [], []
    for _ in range(int(rng.integers(1, 4)) + 1):
        width = int(rng.integers(1, 4))
        rows = []
        for _ in range(int(rng.integers(4, 13))):
            f = int(rng.choice([0, 1, 1, 1, 2, P - 1, 3]))
            rows.append((f, [int(v) for v in rng.integers(0, 3, size=width)]))
        ends.append(rows)
        bits.append(bool(rng.integers(0, 2)))
    return ends, bits


@pytest.mark.parametrize("seed", range(12))
def test_the_model_is_the_headers_definition_on_tiny_links(seed):
    ends, bits = tiny_link(0x5E70 + seed)
    got = model.link_report(ends, bits, False)
    want = brute_force(ends, bits)
    assert {k: got[k] for k in want} == want


def test_the_model_on_cases_small_enough_to_state_by_hand():
    # (1, 2) sent twice and exposed as (1, 2, 0) with multiplicity 2: one value, balanced
    r = model.link_report([[(1, [1, 2]), (0, [9, 9]), (1, [1, 2])], [(2, [1, 2, 0])]], [True, False], True)
    assert r["holds"] and r["n_unbalanced"] == 0 and (r["n_looking"], r["n_looked"]) == (2, 1) and r["first_looking_row"] == -1
    # the second looking end sends a stranger; the exposed (5) is asked for by nobody: two values
    r = model.link_report([[(1, [3])], [(0, [4]), (1, [4])], [(1, [3]), (1, [5])]], [True, True, True], False)
    assert not r["holds"] and r["n_unbalanced"] == 2 and (r["first_looking_end"], r["first_looking_row"], r["first_looked_row"]) == (1, 1, 1)
    # filters 1 and p - 1 on a stranger cancel: balanced, but a bad filter where the port demands a bit
    ends = [[(1, [7]), (P - 1, [7])], [(0, [0])]]
    r = model.link_report(ends, [True, False], True)
    assert not r["holds"] and r["n_unbalanced"] == 0 and (r["bad_filter_end"], r["bad_filter_row"], r["bad_filter_value"]) == (0, 1, P - 1)
    assert model.link_report(ends, [False, False], True)["holds"]
    # the all-zero tuple is the empty value, a value like any other
    assert model.strip([0, 0]) == () and model.link_report([[(1, [0, 0])], [(1, [0])]], [True, True], False)["holds"]


def test_the_model_reads_builders_and_the_memory_table(bpg):
    """report(): a flag table looking words up in AIR 3's columns, as the GPU tests use it"""
    rng = np.random.default_rng(0x5E90)
    mem = np.zeros((45, 16), dtype=np.uint64)
    mem[:11] = rng.integers(0, 1 << 32, size=(11, 16), dtype=np.uint64)
    asked = [2, 7, 11]
    mem[model.MEM_G, asked] = 1
    words = [[int(v) for v in mem[:11, r]] for r in asked]
    b = pc.flag_program(width=11, n_cols=16)
    t = pc.flag_witness(4, [1, 0, 1, 1] + [0] * 12, [words[2], words[0], words[0], words[1]] + [[0] * 11] * 12, width=11, n_cols=16)
    link = [([(0, 0)], (1, 0))]
    r, = model.report([{"builder": b, "trace": t}, {"air_id": 3, "trace": mem}], link)
    assert r["holds"] and (r["n_looking"], r["n_looked"]) == (3, 3) and not r["is_log"]
    t[3, 2] ^= np.uint64(1)
    r, = model.report([{"builder": b, "trace": t}, {"air_id": 3, "trace": mem}], link)
    assert not r["holds"] and r["n_unbalanced"] == 2 and (r["first_looking_end"], r["first_looking_row"], r["first_looked_row"]) == (0, 2, 2)


# ---------------------------------------------------------------------------------------------- 2. the refusals


def test_the_statements_refusals_are_the_provers_and_come_before_any_device_call(bpg):
    """every refusal of check_set through bp_check_table_set, with null device pointers: status -2 and the prover's text
    under the new entry's name"""
    one = bpg.ops.air_register(pc.flag_program(ports=1).assemble())
    two = bpg.ops.air_register(pc.flag_program(ports=2).assemble())
    b = pc.flag_program(ports=1)
    b.log_port(b.loc(0), [b.loc(1)])
    b.log_port(b.loc(2), [b.loc(3)], multiplicity=True)
    mixed = bpg.ops.air_register(b.assemble())
    cfg = lambda air_id, log_n=5: cases.cfg_for(air_id, log_n, num_queries=6, pow_bits=6)
    A, B, C2, M = {"air_id": one, "cfg": cfg(one)}, {"air_id": one, "cfg": cfg(one, 7)}, {"air_id": two, "cfg": cfg(two)}, {"air_id": mixed, "cfg": cfg(mixed)}

    def refused(tables, links, what):
        with pytest.raises(BpgError) as e:
            bpg.ops.check_table_set(tables, links)
        assert e.value.code == -2 and e.value.message.startswith("bp_check_table_set: ") and re.search(what, e.value.message), e.value.message
        # the prover says the same under its own name
        with pytest.raises(BpgError) as p:
            bpg.ops.stark_prove_table_set(tables, links)
        assert p.value.code == -2 and p.value.message == e.value.message.replace("bp_check_table_set", "bp_stark_prove_table_set")

    refused([A, C2], [([(0, 0)], (1, 0))], "port 1 of table 1 is in no link")              # an unlinked port
    refused([A, B, C2], [([(0, 0)], (1, 0)), ([(0, 0)], (2, 0)), ([(2, 1)], (1, 0))], "named twice")  # a port named twice
    refused([A] * 9, [([(0, 0)], (1, 0))], "1 .. 8 tables, got 9")                          # a ninth table
    refused([A, {"air_id": 4, "cfg": cfg(4)}], [([(0, 0)], (1, 0))], "table 1: air_id 4 .* has no lookup port")  # no lookup side
    refused([M, M], [([(0, 0)], (1, 2)), ([(0, 1)], (0, 2)), ([(1, 1)], (1, 0))],
            "link 0 mixes product and log ports: port 2 of table 1 is a log port, port 0 of table 0 a product port")
    refused([A, B], [([(0, 0)], (2, 0))], "names table 2 of 2")
    refused([A, B], [([(0, 1)], (1, 0))], "names port 1 of table 0, which has 1")
    refused([A, B], [([(0, 0)], (1, 0))] * 17, "1 .. 16 links, got 17")
    refused([A, {"air_id": one, "cfg": bpg.ops.stark_cfg(5, 9, num_queries=6, pow_bits=6)}], [([(0, 0)], (1, 0))], "table 1: .*8 columns")
    refused([A, B], [([(0, 0)], (1, 0))], "table 0: null trace")                            # a well-formed statement gets as far as the traces


def test_null_arguments_of_the_entry_are_refused(bpg):
    import ctypes as C
    from proof_protocol_decoder_amd._lib import SetReport
    one = bpg.ops.air_register(pc.flag_program(ports=1).assemble())
    t = {"air_id": one, "cfg": cases.cfg_for(one, 5, num_queries=6, pow_bits=6)}
    ta, la, _ = bpg.ops._set_arguments([t, t], [([(0, 0)], (1, 0))])
    L, rep = bpg.lib(), SetReport()
    assert L.bp_check_table_set(ta, 2, la, 1, 0, None) == -2
    assert L.bp_check_table_set(None, 2, la, 1, 0, C.byref(rep)) == -2
    assert L.bp_check_table_set(ta, 2, None, 1, 0, C.byref(rep)) == -2
    assert L.bp_check_table_set(ta, 2, la, 1, 0, C.byref(rep)) == -2 and b"null trace" in L.bp_last_error()   # (refused before any device call)
    assert C.sizeof(SetReport) == 8 * (16 + 8 * 24) + 16 * 72


# ---------------------------------------------------------------------------------------------- 3. the device source


def test_set_check_kernels_have_no_scratch_and_no_spill(tmp_path):
    from test_build import device_assembly
    asm = device_assembly("set_check.hip", tmp_path)
    name, seen = None, 0
    for line in asm.splitlines():
        m = re.match(r"\s+\.name:\s+(\S+)", line)
        if m:
            name = m.group(1)
            seen += "set_" in name
        m = re.match(r"\s+\.private_segment_fixed_size:\s+(\d+)", line)
        if m:
            assert int(m.group(1)) == 0, (name, "scratch")
        m = re.match(r"\s+\.sgpr_spill_count:\s+(\d+)", line)
        if m:
            assert int(m.group(1)) == 0, (name, int(m.group(1)))
        m = re.match(r"\s+\.vgpr_spill_count:\s+(\d+)", line)
        if m:
            assert int(m.group(1)) == 0, (name, int(m.group(1)))
    assert seen >= 8   # the program's keys, five built-in tables' keys, the clear, the scan


def test_set_check_kernels_have_no_carry_mask_hazard(tmp_path):
    from test_build import device_assembly, scan_carry_mask_hazards
    bad, n = scan_carry_mask_hazards(device_assembly("set_check.hip", tmp_path))
    # n: the scan saw the kernels' field arithmetic (the floor of tests/test_air_program.py's scan; it was 1000 while a
    # built-in port's term was inlined three times per key kernel, with an inversion: one pass over the tuple is less code)
    assert n > 100 and not bad, bad[:10]


def test_set_check_kernels_have_no_dpp_read_of_a_fresh_asm_result(tmp_path):
    """test_build.test_no_dpp_reads_a_fresh_asm_result's rule on set_check.hip (as tests/test_air_check.py applies it to
    air_check.hip)"""
    from test_build import _vregs, device_assembly
    in_asm, recent, bad = False, [], []
    for ln, line in enumerate(device_assembly("set_check.hip", tmp_path).splitlines(), 1):
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
