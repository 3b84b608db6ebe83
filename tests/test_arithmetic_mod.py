"""The modular table on the CPU: the shipped program (proof_protocol_decoder_amd/arithmetic_mod.py) against the
independent row model of tests/arithmetic_mod_model.py -- the column maps, Builder.evaluate over Python integers, the
library's host checker -- and a catalogue of wrong witnesses, each named at its row and family.  Nothing here needs a
GPU; the device side is tests/test_gpu_arithmetic_mod.py."""
import numpy as np
import pytest

import arithmetic_mod_model as model
from proof_protocol_decoder_amd import arithmetic_mod as am
from proof_protocol_decoder_amd.air_program import MAX_FAMILIES_WITH_PORTS, MAX_REGS


@pytest.fixture(scope="module")
def program():
    return am.program()


@pytest.fixture(scope="module")
def reg():
    import proof_protocol_decoder_amd as pkg
    pkg.lib()
    return am.register()


@pytest.fixture(scope="module")
def edge_trace():
    t = model.trace_of(model.edge_ops())
    t.setflags(write=False)
    return t


def test_the_three_column_maps_agree():
    """the module's constants, the kernel's (bp_arithmetic_mod_layout) and the model's, which is written from AIRS.md"""
    assert am.kernel_layout() == am.LAYOUT
    mine = (model.N_COLS, model.IS_ADDMOD, model.IS_MULMOD, model.G, model.Z, model.INV, model.A, model.B_, model.M, model.RES,
            model.Q, model.A_BITS, model.B_BITS, model.M_BITS, model.Q_BITS, model.R_BITS, model.D_BITS, model.CARRY,
            model.CARRY_BITS, model.CARRY_OFFSET, model.BORROW)
    assert mine == am.LAYOUT
    assert [(n, c) for n, c, _ in am.FAMILIES] == model.FAMILIES
    assert len(am.TUPLE_COLS) == 66 and am.N_COLS == 2560


def test_the_layout_entry_refuses_a_short_or_null_buffer():
    import ctypes as C
    import proof_protocol_decoder_amd as pkg
    out = (C.c_uint32 * 32)()
    assert pkg.lib().bp_arithmetic_mod_layout(out, len(am.LAYOUT) - 1) == -2
    assert b"21 words" in pkg.lib().bp_last_error()
    assert pkg.lib().bp_arithmetic_mod_layout(out, 0) == -2 and not any(out)
    assert pkg.lib().bp_arithmetic_mod_layout(None, 32) == -2
    assert pkg.lib().bp_arithmetic_mod_layout(out, 32) == 0 and tuple(out[:len(am.LAYOUT)]) == am.LAYOUT


def test_the_program_fits_the_format_and_registers_once(program, reg):
    import proof_protocol_decoder_amd as pkg
    from proof_protocol_decoder_amd import arithmetic_div as ad
    words = program.assemble()
    assert int(words[0]) == int.from_bytes(b"BPGAIRP2", "little")
    assert int(words[7]) <= MAX_REGS and len(program.units) == 33 <= 256 and len(program.families) == 19 <= MAX_FAMILIES_WITH_PORTS
    assert reg & 0x80000000 and am.register() == reg and pkg.ops.air_register(words) == reg
    assert pkg.lib().bp_air_count() == 9                                       # no built-in was added
    assert ad.register() != reg                                                # ... and the division table keeps its own id
    d = pkg.ops.air_describe(reg)
    assert (d.n_cols, d.degree, d.n_aux, d.n_air_constraints, d.n_units) == (2560, 3, 2, model.N_CONSTRAINTS, 33)
    fams = [(f.first_index, f.count, f.kind, f.degree) for f in d.families[:d.n_families]]
    first = 0
    for (name, count, degree), got in zip(am.FAMILIES, fams):
        assert got == (first, count, 0, degree), name
        assert am.first_index(name) == first
        first += count
    # the library's five constraints of the product port follow the program's own
    assert first == model.N_CONSTRAINTS == 2612 and d.n_families == 19 + 5
    assert sum(f[1] for f in fams[19:]) == 5 == d.n_ctl_constraints and fams[19][0] == first


def test_the_program_vanishes_on_every_model_row(program):
    """every edge triple under both flags, exposed and not, the padding rows, random operations: 2^7 rows"""
    for i, op in enumerate(model.edge_ops_full()):
        row = model.cells(model.honest(*op))
        bad = [k for k, v in enumerate(program.evaluate(row, row)) if v]
        assert not bad, (i, op, [model.family_of(k) for k in bad[:4]])
        (f, tup), = program.evaluate_ports(row, row)
        want_g = int(op[0] in (model.ADDMOD, model.MULMOD) and bool(op[4]))
        assert f == want_g and len(tup) == 66 and tup == [row[c] for c in am.TUPLE_COLS]


def test_a_padding_row_is_zero_but_for_z_and_the_carry_offsets():
    row = model.cells(model.honest(*model.PADDING[0]))
    offsets = {model.CARRY + model.CARRY_BITS * k + 20 for k in range(31)}
    assert {c for c, v in enumerate(row) if v} == {model.Z} | offsets and all(row[c] == 1 for c in offsets)


def test_both_carry_extremes_are_reached_and_fit():
    """AIRS.md: each side's own carry is at most 16 (2^16 - 1) + 1, so |c_k| < 2^20"""
    assert 16 * (model.B - 1) + 1 < model.CARRY_OFFSET == 1 << (model.CARRY_BITS - 1)
    lo = model.honest(model.MULMOD, *model.MOST_NEGATIVE, 1)["signed_carry"]
    hi = model.honest(model.MULMOD, *model.MOST_POSITIVE, 1)["signed_carry"]
    assert min(lo) == -0xEFFF1 and max(hi) == hi[15] == 0xFFFEF
    for op in model.edge_ops_full() + model.random_ops(1500, 0xCA45):
        c = model.honest(*op)["signed_carry"]
        assert -0xEFFF1 <= min(c) and max(c) <= 0xFFFEF, op


def test_the_model_rows_state_the_evm_operations():
    """the model against the statement itself: (a + b) % m and (a * b) % m, zero for m = 0"""
    for op, a, b, m, e in model.edge_ops_full():
        w = model.honest(op, a, b, m, e)
        if op not in (model.ADDMOD, model.MULMOD):
            assert model.word(w["resl"]) == 0 and w["g"] == 0
            continue
        u = a + b if op == model.ADDMOD else a * b
        assert model.word(w["resl"]) == (u % m if m else 0)
        assert model.word(w["ql"]) * (m if m else 1 << 256) + w["rb"] == u and (w["rb"] < m or not m)


def test_the_host_checker_is_clean_on_the_model_trace(reg, edge_trace):
    import proof_protocol_decoder_amd as pkg
    assert edge_trace.shape == (2560, 32)
    got = pkg.ops.check_air_trace_host(reg, edge_trace)
    assert got.ok and got.n_violations == 0, got


def test_unpack_row_and_pack_inputs_give_back_the_operations(edge_trace):
    ops = model.edge_ops()
    words = am.pack_inputs(ops)
    assert words.shape == (32, 13) and words.dtype == np.uint64
    for i, (op, a, b, m, exposed) in enumerate(ops):
        assert int(words[i, 0]) == op | (bool(exposed) << 8)
        for first, v in ((1, a), (5, b), (9, m)):
            assert sum(int(words[i, first + k]) << (64 * k) for k in range(4)) == v
        got = am.unpack_row(edge_trace, i)
        if op not in (model.ADDMOD, model.MULMOD):
            assert got == (0, 0, 0, 0, 0, 0, 0, 0)
            continue
        u = a + b if op == model.ADDMOD else a * b
        q, r = divmod(u, m) if m else (u >> 256, u & model.M256)
        assert got == (op, a, b, m, q, r, r if m else 0, int(bool(exposed)))
    with pytest.raises(ValueError):
        am.pack_inputs([(1, 1, 1, 1 << 256, 0)])


@pytest.mark.parametrize("entry", model.CATALOGUE, ids=[e[0] for e in model.CATALOGUE])
def test_a_wrong_witness_is_named_at_its_row_and_family(program, reg, edge_trace, entry):
    """the forged row replaces row 9 of the edge trace; Python integers and the host checker name the same constraints,
    all of them in the families the forgery means to break"""
    import proof_protocol_decoder_amd as pkg
    name, _, _, families = entry
    row = model.forged(entry)
    broken = [k for k, v in enumerate(program.evaluate(row, row)) if v]
    assert broken and {model.family_of(k)[1] for k in broken} == families, (name, [model.family_of(k) for k in broken])
    t = edge_trace.copy()
    t[:, 9] = np.array(row, dtype=np.uint64)
    got = pkg.ops.check_air_trace_host(reg, t, max_viol=512)
    assert got.n_violated_rows == 1 and got.rows == [9] and got.n_violations == len(broken)
    assert sorted(v.constraint for v in got.violations) == broken and {v.row for v in got.violations} == {9}
    assert {am.FAMILIES[v.family][0] for v in got.violations} == families
    assert all(model.family_of(v.constraint)[0] == v.family for v in got.violations)


def test_the_wrapped_sum_breaks_the_first_column_above_the_low_half(program):
    """ADDMOD from (a + b) mod 2^256: columns 0 .. 15 add up, column 16 is where the missing 2^256 shows"""
    row = model.forged(model.CATALOGUE[0])
    broken = [k for k, v in enumerate(program.evaluate(row, row)) if v]
    assert broken == [am.first_index("product") + 16]
