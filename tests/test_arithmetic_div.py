"""The division table on the CPU: the shipped program (proof_protocol_decoder_amd/arithmetic_div.py) against the
independent row model of tests/arithmetic_div_model.py -- the column maps, Builder.evaluate over Python integers, the
library's host checker -- and a catalogue of wrong witnesses, each named at its row and family.  Nothing here needs a
GPU; the device side is tests/test_gpu_arithmetic_div.py."""
import numpy as np
import pytest

import arithmetic_div_model as model
from proof_protocol_decoder_amd import arithmetic_div as ad
from proof_protocol_decoder_amd.air_program import MAX_FAMILIES_WITH_PORTS, MAX_REGS


@pytest.fixture(scope="module")
def program():
    return ad.program()


@pytest.fixture(scope="module")
def reg():
    import proof_protocol_decoder_amd as pkg
    pkg.lib()
    return ad.register()


@pytest.fixture(scope="module")
def edge_trace():
    t = model.trace_of(model.edge_ops())
    t.setflags(write=False)
    return t


def test_the_three_column_maps_agree():
    """the module's constants, the kernel's (bp_arithmetic_div_layout) and the model's, which is written from AIRS.md"""
    assert ad.kernel_layout() == ad.LAYOUT
    mine = (model.N_COLS, model.IS_DIV, model.IS_MOD, model.G, model.Z, model.INV, model.X, model.Y, model.RES, model.Q,
            model.X_BITS, model.Y_BITS, model.Q_BITS, model.R_BITS, model.D_BITS, model.CARRY, model.CARRY_BITS, model.BORROW)
    assert mine == ad.LAYOUT
    assert [(n, c) for n, c, _ in ad.FAMILIES] == model.FAMILIES
    assert len(ad.TUPLE_COLS) == 50 and ad.N_COLS == 1650


def test_the_layout_entry_refuses_a_short_buffer():
    import ctypes as C
    import proof_protocol_decoder_amd as pkg
    out = (C.c_uint32 * 32)()
    assert pkg.lib().bp_arithmetic_div_layout(out, len(ad.LAYOUT) - 1) == -2
    assert pkg.lib().bp_arithmetic_div_layout(None, 32) == -2
    assert pkg.lib().bp_arithmetic_div_layout(out, 32) == 0 and tuple(out[:len(ad.LAYOUT)]) == ad.LAYOUT


def test_the_program_fits_the_format_and_registers_once(program, reg):
    import proof_protocol_decoder_amd as pkg
    words = program.assemble()
    assert int(words[0]) == int.from_bytes(b"BPGAIRP2", "little")
    assert int(words[7]) <= MAX_REGS and len(program.units) == 9 <= 256 and len(program.families) == 19 <= MAX_FAMILIES_WITH_PORTS
    assert reg & 0x80000000 and ad.register() == reg and pkg.ops.air_register(words) == reg
    assert pkg.lib().bp_air_count() == 9                                       # no built-in was added
    d = pkg.ops.air_describe(reg)
    assert (d.n_cols, d.degree, d.n_aux, d.n_air_constraints, d.n_units) == (1650, 3, 2, model.N_CONSTRAINTS, 9)
    fams = [(f.first_index, f.count, f.kind, f.degree) for f in d.families[:d.n_families]]
    first = 0
    for (name, count, degree), got in zip(ad.FAMILIES, fams):
        assert got == (first, count, 0, degree), name
        assert ad.first_index(name) == first
        first += count
    # the library's five constraints of the product port follow the program's own
    assert first == model.N_CONSTRAINTS and d.n_families == 19 + 5
    assert sum(f[1] for f in fams[19:]) == 5 == d.n_ctl_constraints and fams[19][0] == first


def test_the_program_vanishes_on_every_model_row(program):
    """every edge pair under both flags, exposed and not, the padding rows, random operands: 2^7 rows"""
    for i, op in enumerate(model.edge_ops_full()):
        row = model.cells(model.honest(*op))
        bad = [k for k, v in enumerate(program.evaluate(row, row)) if v]
        assert not bad, (i, op, [model.family_of(k) for k in bad[:4]])
        (f, tup), = program.evaluate_ports(row, row)
        want_g = int(op[0] in (model.DIV, model.MOD) and bool(op[3]))
        assert f == want_g and len(tup) == 50 and tup == [row[c] for c in ad.TUPLE_COLS]


def test_the_largest_carry_is_reached_and_fits():
    w = model.honest(model.DIV, *model.LARGEST_CARRY, 1)
    assert max(w["carry"]) == w["carry"][7] == 0x7FFF7 and 1 << 18 <= 0x7FFF7 < 1 << model.CARRY_BITS
    # the bound in include/bpg.h: at most eight products that are not zero in a column
    assert 8 * (model.B - 1) + 1 < 1 << model.CARRY_BITS
    for op in model.edge_ops_full() + model.random_ops(2000, 0xCA44):
        w = model.honest(*op)
        assert max(w["carry"]) <= 0x7FFF7, op


def test_the_host_checker_is_clean_on_the_model_trace(reg, edge_trace):
    import proof_protocol_decoder_amd as pkg
    assert edge_trace.shape == (1650, 32)
    got = pkg.ops.check_air_trace_host(reg, edge_trace)
    assert got.ok and got.n_violations == 0, got


def test_unpack_row_and_pack_inputs_give_back_divmod(edge_trace):
    ops = model.edge_ops()
    words = ad.pack_inputs(ops)
    assert words.shape == (32, 9) and words.dtype == np.uint64
    for i, (op, x, y, exposed) in enumerate(ops):
        assert int(words[i, 0]) == op | (bool(exposed) << 8)
        assert sum(int(words[i, 1 + k]) << (64 * k) for k in range(4)) == x
        assert sum(int(words[i, 5 + k]) << (64 * k) for k in range(4)) == y
        got = ad.unpack_row(edge_trace, i)
        if op not in (model.DIV, model.MOD):
            assert got == (0, 0, 0, 0, 0, 0, 0)
            continue
        q, r = divmod(x, y) if y else (0, x)
        assert got == (op, x, y, q, r, 0 if y == 0 else (q if op == model.DIV else r), int(bool(exposed)))
    with pytest.raises(ValueError):
        ad.pack_inputs([(1, 1 << 256, 1, 0)])


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
    assert {ad.FAMILIES[v.family][0] for v in got.violations} == families
    assert all(model.family_of(v.constraint)[0] == v.family for v in got.violations)
