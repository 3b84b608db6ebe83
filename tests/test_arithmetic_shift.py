"""The shift table on the CPU: the shipped program (proof_protocol_decoder_amd/arithmetic_shift.py) against the
independent row model of tests/arithmetic_shift_model.py -- the column maps, Builder.evaluate over Python integers, the
library's host checker -- and a catalogue of wrong witnesses, each named at its row and family.  The bodies restate
word_tables.cpu_tests for a table of three operations and sixteen families.  Nothing here needs a GPU; the device side
is tests/test_gpu_arithmetic_shift.py."""
import numpy as np
import pytest

import arithmetic_shift_model as model
from proof_protocol_decoder_amd import arithmetic_div, arithmetic_mod, arithmetic_shift as sh
from proof_protocol_decoder_amd.air_program import MAX_FAMILIES_WITH_PORTS, MAX_REGS

N_COLS, WIDTH, LAYOUT_WORDS, N_FAMILIES, N_CONSTRAINTS, N_UNITS = 1143, 51, 19, 16, 1165, 17   # AIRS.md section 2
MODEL_LAYOUT = (model.N_COLS, model.IS_SHL, model.IS_SHR, model.IS_SAR, model.G, model.Z, model.INV, model.FILL, model.W,
                model.S, model.X, model.RES, model.Y, model.L, model.E, model.S_BITS, model.X_BITS, model.LO_BITS, model.HI_BITS)


@pytest.fixture(scope="module")
def program():
    return sh.program()


@pytest.fixture(scope="module")
def reg():
    import proof_protocol_decoder_amd as pkg
    pkg.lib()
    return sh.register()


@pytest.fixture(scope="module")
def edge_trace():
    t = model.trace_of(model.edge_ops())
    t.setflags(write=False)
    return t


def test_the_three_column_maps_agree():
    """the module's constants, the kernel's (its layout entry) and the model's, which is written from AIRS.md"""
    assert sh.kernel_layout() == sh.LAYOUT
    assert MODEL_LAYOUT == sh.LAYOUT and len(sh.LAYOUT) == LAYOUT_WORDS
    assert [(n, c) for n, c, _ in sh.FAMILIES] == model.FAMILIES
    assert len(sh.TUPLE_COLS) == WIDTH and sh.N_COLS == N_COLS == model.N_COLS
    assert (sh.SHL, sh.SHR, sh.SAR) == (model.SHL, model.SHR, model.SAR) == (1, 2, 3)


def test_the_layout_entry_refuses_a_short_or_null_buffer():
    import ctypes as C
    import proof_protocol_decoder_amd as pkg
    entry = pkg.lib().bp_arithmetic_shift_layout
    out = (C.c_uint32 * 32)()
    assert entry(out, len(sh.LAYOUT) - 1) == -2
    assert b"%d words" % LAYOUT_WORDS in pkg.lib().bp_last_error()
    assert entry(out, 0) == -2 and not any(out)
    assert entry(None, 32) == -2
    assert entry(out, 32) == 0 and tuple(out[:len(sh.LAYOUT)]) == sh.LAYOUT


def test_the_program_fits_the_format_and_registers_once(program, reg):
    import proof_protocol_decoder_amd as pkg
    words = program.assemble()
    assert int(words[0]) == int.from_bytes(b"BPGAIRP2", "little")
    assert int(words[7]) <= MAX_REGS and len(program.units) == N_UNITS <= 256
    assert len(program.families) == N_FAMILIES <= MAX_FAMILIES_WITH_PORTS
    assert reg & 0x80000000 and sh.register() == reg and pkg.ops.air_register(words) == reg
    assert pkg.lib().bp_air_count() == 9                                       # no built-in was added
    assert len({reg, arithmetic_div.register(), arithmetic_mod.register()}) == 3   # ... and every table keeps its own id
    d = pkg.ops.air_describe(reg)
    assert (d.n_cols, d.degree, d.n_aux, d.n_air_constraints, d.n_units) == (N_COLS, 3, 2, model.N_CONSTRAINTS, N_UNITS)
    fams = [(f.first_index, f.count, f.kind, f.degree) for f in d.families[:d.n_families]]
    first = 0
    for (name, count, degree), got in zip(sh.FAMILIES, fams):
        assert got == (first, count, 0, degree), name
        assert sh.first_index(name) == first
        first += count
    # the library's five constraints of the product port follow the program's own
    assert first == model.N_CONSTRAINTS == N_CONSTRAINTS and d.n_families == N_FAMILIES + 5
    assert sum(f[1] for f in fams[N_FAMILIES:]) == 5 == d.n_ctl_constraints and fams[N_FAMILIES][0] == first


def test_every_unit_cut_states_the_same_constraints():
    row = model.cells(model.honest(model.SAR, 0x47, model.G1, 1))
    bad = model.forged(model.CATALOGUE[7])
    want = sh.program().evaluate(bad, bad)
    assert any(want)
    for cut in sh.CUTS:
        p = sh.program(cut)
        # a register is 2 KiB of a workgroup's LDS: the shipped cut needs no more than the division table's 8
        assert len(p.units) == 1 + 16 // cut and int(p.assemble()[7]) <= (8 if cut == sh.LIMBS_PER_UNIT else 16)
        assert not any(p.evaluate(row, row)) and p.evaluate(bad, bad) == want
    with pytest.raises(ValueError):
        sh.program(3)


def test_the_edge_list_covers_what_the_statement_singles_out():
    ops = model.edge_ops()
    assert len(ops) == 32 and len(model.edge_ops_full()) == 128
    assert all(ops[i][0] not in model.LIVE for i in model.PADDING_ROWS) and 9 in model.PADDING_ROWS
    for collection in (ops, model.edge_ops_full()):
        counts, values = {o[1] for o in collection if o[0] in model.LIVE}, {o[2] for o in collection if o[0] in model.LIVE}
        assert {0, 1, 15, 16, 17, 255, 256, 257, 0x300, (1 << 16) + 5, 1 << 255, model.MAX} <= counts
        assert {0, 1, 1 << 255, (1 << 255) - 1, model.MAX} <= values
        sar_negative = {o[1] for o in collection if o[0] == model.SAR and o[2] >> 255}
        assert 255 in sar_negative and any(s >= 256 for s in sar_negative)
    below = sum(1 for o in model.random_ops(1000, 1) if o[1] < 256)
    assert 450 < below < 650                                   # half the draws, and the short words of the other half


def test_the_program_vanishes_on_every_model_row(program):
    """every edge under all three flags, exposed and not, the padding rows, random operations: 2^7 rows"""
    for i, op in enumerate(model.edge_ops_full()):
        row = model.cells(model.honest(*op))
        bad = [k for k, v in enumerate(program.evaluate(row, row)) if v]
        assert not bad, (i, op, [model.family_of(k) for k in bad[:4]])
        (f, tup), = program.evaluate_ports(row, row)
        want_g = int(op[0] in model.LIVE and bool(op[3]))
        assert f == want_g == row[model.G] and len(tup) == WIDTH and tup == [row[c] for c in sh.TUPLE_COLS]
        assert tup == [int(op[0] == o) for o in model.LIVE] + row[model.S:model.S + 48]


def test_the_model_rows_state_the_evm_operations():
    """the model's limb-wise witness against the statement itself, and the masked count giving another answer"""
    for op, s, x, e in model.edge_ops_full() + model.random_ops(400, 0x5F72):
        w = model.honest(op, s, x, e)
        if op not in model.LIVE:
            assert model.word(w["resl"]) == model.word(w["sl"]) == model.word(w["xl"]) == 0 and w["g"] == 0
            assert (w["z"], w["l"][0], w["e"][15], w["W"]) == (1, 1, 1, 0) and not any(w["y"] + w["lo"] + w["hi"])
            continue
        signed = x - (x >> 255 << 256)
        want = {model.SHL: (x << min(s, 256)) & model.M256, model.SHR: x >> min(s, 256), model.SAR: (signed >> min(s, 256)) & model.M256}[op]
        assert model.word(w["resl"]) == want == model.statement(op, s, x)
    assert model.statement(model.SHL, 256, 5) == 0 != model.statement(model.SHL, 0, 5)


def test_the_largest_values_are_below_the_field(program):
    """AIRS.md: x_k W < 2^32, T < 2^20, |sum d e_d| <= 15 -- the edge rows reach the first two"""
    w = model.honest(model.SHR, model.MAX, model.MAX, 1)
    assert w["W"] == 2 and sum(w["sl"][1:]) + 0xFF == 15 * 0xFFFF + 0xFF < 1 << 20
    w = model.honest(model.SAR, 0, model.MAX, 1)
    assert w["W"] == 1 << 16 and max(xk * w["W"] for xk in w["xl"]) == 0xFFFF0000 < model.P


def test_the_host_checker_is_clean_on_the_model_trace(reg, edge_trace):
    import proof_protocol_decoder_amd as pkg
    assert edge_trace.shape == (N_COLS, 32)
    got = pkg.ops.check_air_trace_host(reg, edge_trace)
    assert got.ok and got.n_violations == 0, got


def test_unpack_row_and_pack_inputs_give_back_the_operations(edge_trace):
    """(op, s, x, res, g) of every row of the edge list, against the statement"""
    ops = model.edge_ops()
    words = sh.pack_inputs(ops)
    assert words.shape == (32, 9) and words.dtype == np.uint64
    for i, (op, s, x, exposed) in enumerate(ops):
        assert int(words[i, 0]) == op | (bool(exposed) << 8)
        for j, v in enumerate((s, x)):
            assert sum(int(words[i, 1 + 4 * j + k]) << (64 * k) for k in range(4)) == v
        got = sh.unpack_row(edge_trace, i)
        if op not in model.LIVE:
            assert got == (0, 0, 0, 0, 0)
            continue
        assert got == (op, s, x, model.statement(op, s, x), int(bool(exposed)))
    with pytest.raises(ValueError):
        sh.pack_inputs([(1, 1 << 256, 1, 0)])


def test_the_catalogue_breaks_every_family():
    assert set().union(*(e[3] for e in model.CATALOGUE)) == {name for name, _ in model.FAMILIES}


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
    assert {sh.FAMILIES[v.family][0] for v in got.violations} == families
    assert all(model.family_of(v.constraint)[0] == v.family for v in got.violations)
