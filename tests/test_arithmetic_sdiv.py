"""The signed table on the CPU: the shipped program (proof_protocol_decoder_amd/arithmetic_sdiv.py) against the
independent row model of tests/arithmetic_sdiv_model.py -- the column maps, Builder.evaluate over Python integers, the
library's host checker -- and a catalogue of wrong witnesses, each named at its row and family.  The bodies restate
word_tables.cpu_tests for this table's record (four shipped tables, its own family count).  Nothing here needs a GPU; the
device side is tests/test_gpu_arithmetic_sdiv.py."""
import math
from fractions import Fraction

import numpy as np
import pytest

import arithmetic_sdiv_model as model
from proof_protocol_decoder_amd import arithmetic_div, arithmetic_mod, arithmetic_sdiv as sd, arithmetic_shift
from proof_protocol_decoder_amd.air_program import MAX_FAMILIES_WITH_PORTS, MAX_REGS

N_COLS, WIDTH, LAYOUT_WORDS, N_FAMILIES, N_CONSTRAINTS, N_UNITS = 2499, 50, 27, 19, 2583, 17   # AIRS.md section 2
MODEL_LAYOUT = (model.N_COLS, model.IS_SDIV, model.IS_SMOD, model.G, model.Z, model.INV, model.NEG, model.X, model.Y, model.RES,
                model.Q, model.AY, model.M, model.X_BITS, model.Y_BITS, model.RES_BITS, model.AX_BITS, model.AY_BITS, model.Q_BITS,
                model.R_BITS, model.D_BITS, model.CARRY, model.CARRY_BITS, model.BORROW, model.X_CHAIN, model.Y_CHAIN,
                model.RES_CHAIN)


@pytest.fixture(scope="module")
def program():
    return sd.program()


@pytest.fixture(scope="module")
def reg():
    import proof_protocol_decoder_amd as pkg
    pkg.lib()
    return sd.register()


@pytest.fixture(scope="module")
def edge_trace():
    t = model.trace_of(model.edge_ops())
    t.setflags(write=False)
    return t


def signed(v):
    return v - (v >> 255 << 256)


def test_the_three_column_maps_agree():
    """the module's constants, the kernel's (its layout entry) and the model's, which is written from AIRS.md"""
    assert sd.kernel_layout() == sd.LAYOUT
    assert MODEL_LAYOUT == sd.LAYOUT and len(sd.LAYOUT) == LAYOUT_WORDS
    assert [(n, c) for n, c, _ in sd.FAMILIES] == model.FAMILIES
    assert len(sd.TUPLE_COLS) == WIDTH and sd.N_COLS == N_COLS == model.N_COLS
    assert (sd.OP_SDIV, sd.OP_SMOD) == (model.SDIV, model.SMOD) == (1, 2)
    # the division table's port: the same flags-and-three-words tuple, so a table that looks divisions up fits this one
    assert len(arithmetic_div.TUPLE_COLS) == WIDTH


def test_the_layout_entry_refuses_a_short_or_null_buffer():
    import ctypes as C
    import proof_protocol_decoder_amd as pkg
    entry = pkg.lib().bp_arithmetic_sdiv_layout
    out = (C.c_uint32 * 32)()
    assert entry(out, len(sd.LAYOUT) - 1) == -2
    assert b"%d words" % LAYOUT_WORDS in pkg.lib().bp_last_error()
    assert entry(out, 0) == -2 and not any(out)
    assert entry(None, 32) == -2
    assert entry(out, 32) == 0 and tuple(out[:len(sd.LAYOUT)]) == sd.LAYOUT


def test_the_program_fits_the_format_and_registers_once(program, reg):
    import proof_protocol_decoder_amd as pkg
    words = program.assemble()
    assert int(words[0]) == int.from_bytes(b"BPGAIRP2", "little")
    assert int(words[7]) <= MAX_REGS and len(program.units) == N_UNITS <= 256
    assert len(program.families) == N_FAMILIES <= MAX_FAMILIES_WITH_PORTS
    assert reg & 0x80000000 and sd.register() == reg and pkg.ops.air_register(words) == reg
    assert pkg.lib().bp_air_count() == 9                                       # no built-in was added
    others = {arithmetic_div.register(), arithmetic_mod.register(), arithmetic_shift.register()}
    assert len(others | {reg}) == 4                                            # ... and every table keeps its own id
    d = pkg.ops.air_describe(reg)
    assert (d.n_cols, d.degree, d.n_aux, d.n_air_constraints, d.n_units) == (N_COLS, 3, 2, model.N_CONSTRAINTS, N_UNITS)
    fams = [(f.first_index, f.count, f.kind, f.degree) for f in d.families[:d.n_families]]
    first = 0
    for (name, count, degree), got in zip(sd.FAMILIES, fams):
        assert got == (first, count, 0, degree), name
        assert sd.first_index(name) == first
        first += count
    # the library's five constraints of the product port follow the program's own
    assert first == model.N_CONSTRAINTS == N_CONSTRAINTS and d.n_families == N_FAMILIES + 5
    assert sum(f[1] for f in fams[N_FAMILIES:]) == 5 == d.n_ctl_constraints and fams[N_FAMILIES][0] == first


def test_every_unit_cut_states_the_same_constraints():
    row = model.cells(model.honest(model.SMOD, model.to_word(-model.EXTREME), model.HALF, 1))
    bad = model.forged(model.CATALOGUE[0])
    want = sd.program().evaluate(bad, bad)
    assert any(want)
    assert sd.CUTS == (1, 2) and sd.LIMBS_PER_UNIT in sd.CUTS
    for cut in sd.CUTS:
        p = sd.program(cut)
        # a register is 2 KiB of a workgroup's LDS: no cut needs more than 16
        assert len(p.units) == 1 + 16 // cut and int(p.assemble()[7]) <= 16
        assert not any(p.evaluate(row, row)) and p.evaluate(bad, bad) == want
    with pytest.raises(ValueError):
        sd.program(4)


def test_the_edge_list_covers_what_the_statement_singles_out():
    ops = model.edge_ops()
    assert len(ops) == 32 and len(model.edge_ops_full()) == 128
    assert all(ops[i][0] not in model.LIVE for i in model.PADDING_ROWS) and 9 in model.PADDING_ROWS
    n_ = model.to_word
    operands = {0, 1, 2, 7, n_(-1), n_(-2), n_(-7), (1 << 255) - 1, 1 << 255, n_(1 - (1 << 255)), model.HALF, n_(-model.HALF),
                1 << 128, n_(-(1 << 128))}
    rows = {(1 << 255, n_(-1)), (1 << 255, 1), (n_(-7), 2), (7, n_(-2)), (n_(-7), n_(-2)), (n_(-8), 2), (n_(-1), 1 << 255),
            (model.EXTREME, model.HALF), (n_(-model.EXTREME), model.HALF)}
    for collection in (ops, model.edge_ops_full()):
        live = [o for o in collection if o[0] in model.LIVE]
        assert operands <= {o[1] for o in live} and operands <= {o[2] for o in live}      # every edge operand in both positions
        assert rows <= {o[1:3] for o in live}
        assert {o[1] >> 255 for o in live if o[2] == 0} == {0, 1}                          # (x, 0) under both signs of x
        assert {o[0] for o in live} == set(model.LIVE)
    full = model.edge_ops_full()
    assert all((op, x, y, e) in full for x, y in model.EDGE_PAIRS for op in model.LIVE for e in (0, 1))
    negative = sum(1 for o in model.random_ops(1000, 1) if o[1] >> 255)
    assert 400 < negative < 600


def test_the_program_vanishes_on_every_model_row(program):
    """every edge under both flags, exposed and not, the padding rows, random operations: 2^7 rows"""
    for i, op in enumerate(model.edge_ops_full()):
        row = model.cells(model.honest(*op))
        bad = [k for k, v in enumerate(program.evaluate(row, row)) if v]
        assert not bad, (i, op, [model.family_of(k) for k in bad[:4]])
        (f, tup), = program.evaluate_ports(row, row)
        want_g = int(op[0] in model.LIVE and bool(op[3]))
        assert f == want_g == row[model.G] and len(tup) == WIDTH and tup == [row[c] for c in sd.TUPLE_COLS]
        if op[0] in model.LIVE:
            want = [int(op[0] == o) for o in model.LIVE] + model.limbs(op[1]) + model.limbs(op[2]) + model.limbs(model.statement(*op[:3]))
            assert tup == want
        else:   # a padding row, as the kernel writes it: all zero except z = 1
            assert [c for c, v in enumerate(row) if v] == [model.Z] and row[model.Z] == 1


def test_the_model_rows_state_the_evm_operations():
    """the model's witness, which divides magnitudes, against the statement written a second way: Python's signed
    integers and an explicit truncation toward zero (never //, which floors)"""
    for op, x, y, e in model.edge_ops_full() + model.random_ops(400, 0x5D12):
        w = model.honest(op, x, y, e)
        res = model.word(w["resl"])
        if op not in model.LIVE:
            assert res == model.word(w["xl"]) == model.word(w["yl"]) == 0 and (w["g"], w["z"], w["neg"]) == (0, 1, 0)
            continue
        sx, sy = signed(x), signed(y)
        if sy == 0:
            assert res == 0 and w["z"] == 1
            continue
        quotient = math.trunc(Fraction(sx, sy))
        remainder = sx - sy * quotient
        assert abs(remainder) < abs(sy) and (remainder == 0 or (remainder < 0) == (sx < 0))   # the sign of the dividend
        assert res == (quotient if op == model.SDIV else remainder) % (1 << 256) == model.statement(op, x, y)
        assert model.word(w["ql"]) == abs(quotient) and w["rb"] == abs(remainder)
    n_ = model.to_word
    # the two classic mistakes, and the quotient that has no positive word
    assert signed(model.statement(model.SDIV, n_(-7), 2)) == -3 != -7 // 2
    assert signed(model.statement(model.SMOD, n_(-7), 2)) == -1 != -7 % 2
    assert signed(model.statement(model.SMOD, 7, n_(-2))) == 1 != 7 % -2
    assert model.statement(model.SDIV, 1 << 255, n_(-1)) == 1 << 255 and model.statement(model.SMOD, 1 << 255, n_(-1)) == 0
    assert model.statement(model.SDIV, n_(-8), 2) == n_(-4) and model.statement(model.SMOD, n_(-8), 2) == 0
    assert model.statement(model.SDIV, 5, 0) == model.statement(model.SMOD, n_(-5), 0) == 0


def test_the_largest_values_are_below_the_field():
    """AIRS.md: the largest carry a search found, 0x77FF8 out of column 7 under either sign of x, needs all 19 bits; a
    product column stays below 2^37, a chain limb below 2^18"""
    for x in (model.EXTREME, model.to_word(-model.EXTREME)):
        w = model.honest(model.SDIV, x, model.HALF, 1)
        assert max(w["carry"]) == w["carry"][7] == model.LARGEST_CARRY and model.LARGEST_CARRY >> 18 == 1
        assert w["rb"] == model.HALF - 1 and model.word(w["ql"]) == (1 << 127) - 1
    assert max(max(model.honest(*op)["carry"]) for op in model.edge_ops_full() + model.random_ops(400, 0x5D13)) == model.LARGEST_CARRY
    assert 16 * 0xFFFF * 0xFFFF + 0xFFFF + (1 << 19) < 1 << 37 < model.P and 2 * 0xFFFF + 1 < 1 << 18
    w = model.honest(model.SDIV, 1 << 255, model.to_word(-1), 1)               # the magnitude 2^255, which no positive word holds
    assert w["axb"] == 1 << 255 == w["qb"] == w["resb"] and w["neg"] == 0 and w["cx"][15] == 1


def test_the_host_checker_is_clean_on_the_model_trace(reg, edge_trace):
    import proof_protocol_decoder_amd as pkg
    assert edge_trace.shape == (N_COLS, 32)
    got = pkg.ops.check_air_trace_host(reg, edge_trace)
    assert got.ok and got.n_violations == 0, got


def test_unpack_row_and_pack_inputs_give_back_the_operations(edge_trace):
    """(op, x, y, q, r, res, g) of every row of the edge list, against the statement"""
    ops = model.edge_ops()
    words = sd.pack_inputs(ops)
    assert words.shape == (32, 9) and words.dtype == np.uint64
    assert (words == arithmetic_div.pack_inputs(ops)).all()                    # the division table's input format
    for i, (op, x, y, exposed) in enumerate(ops):
        assert int(words[i, 0]) == op | (bool(exposed) << 8)
        for j, v in enumerate((x, y)):
            assert sum(int(words[i, 1 + 4 * j + k]) << (64 * k) for k in range(4)) == v
        got = sd.unpack_row(edge_trace, i)
        if op not in model.LIVE:
            assert got == (0,) * 7
            continue
        ax, ay = abs(signed(x)), abs(signed(y))
        q, r = divmod(ax, ay) if ay else (0, ax)
        assert got == (op, x, y, q, r, model.statement(op, x, y), int(bool(exposed)))
    with pytest.raises(ValueError):
        sd.pack_inputs([(1, 1 << 256, 1, 0)])


def test_the_catalogue_breaks_every_family():
    assert set().union(*(e[3] for e in model.CATALOGUE)) == {name for name, _ in model.FAMILIES}
    assert len({e[0] for e in model.CATALOGUE}) == len(model.CATALOGUE)


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
    assert {sd.FAMILIES[v.family][0] for v in got.violations} == families
    assert all(model.family_of(v.constraint)[0] == v.family for v in got.violations)
