"""What the tests know about the five shipped tables over 256-bit words -- division, modular, shift, signed and
exponentiation --, stated once.  A plain module, not collected, in the manner of tests/builtin_airs.py.

DIVISION, MODULAR, SHIFT, SIGNED and EXPONENTIATION are one record per table, TABLES all five: the package module, the
independent model, the entry names, and as literals the shapes AIRS.md section 2 states (columns, port width, units,
families, constraints), the seeds, the lists the device witness is compared on and the rows its table-set scenario asks
for.  A body below reads the record and nothing else about its table: the op bytes are the model's LIVE, the tuple has a
flag for each, and what unpack_row gives between the operands and g is what the record's `answers` returns.

The bodies come in two layers.  program_tests (CPU) and proof_tests (GPU) hold for every table: the layout entry, the
program's format and registration, the proof of the 2^5-row trace, the port's running products.  cpu_tests and gpu_tests
add what holds for a table of one operation per row, where a forgery is a row and the inputs are one tensor; the
exponentiation table, whose operations span rows, binds the first layer and keeps bodies of its own for the rest.  Each
returns {name: fixture or test}, which a test file puts into its globals -- renamed(...) where the file says "divisions"
for "the operations" -- before the tests that are its table's own.  Last, the helpers of the table-set stories each GPU
file tells for itself."""
from types import SimpleNamespace

import numpy as np
import pytest

import arithmetic_div_model
import arithmetic_exp_model
import arithmetic_mod_model
import arithmetic_sdiv_model
import arithmetic_shift_model
from proof_protocol_decoder_amd import arithmetic_div, arithmetic_exp, arithmetic_mod, arithmetic_sdiv, arithmetic_shift
from proof_protocol_decoder_amd.air_program import ALL_ROWS, LAST_ROW, MAX_FAMILIES_WITH_PORTS, MAX_REGS, TRANSITION


def signed(v):
    """the integer a two's-complement word stands for"""
    return v - (v >> 255 << 256)


def dev_starts(starts):
    """the exponentiation table's prefix sums as the int32 device tensor its entry takes"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(starts).view(np.int32)).cuda()


# ---------------------------------------------------------------------------------------------- the records
def _record(name, module, model, stem, **own):
    """what every record has: the entry names, all made of `stem`; then the table's own literals and callables"""
    return SimpleNamespace(name=name, module=module, model=model, layout_entry="bp_%s_layout" % stem,
                           trace_entry="bp_%s_trace" % stem, trace_op="%s_trace" % stem, **own)


def _row_table(name, module, model, stem, **own):
    """a table of one operation per row: 2^log_n operations are a trace, the inputs are pack_inputs' one tensor, every
    family is of kind ALL_ROWS, and the port's tuple is a flag per live op, then the limbs of the operands and the result"""
    def device_trace(bpg, ops, log_n):
        from util import to_dev
        assert len(ops) == 1 << log_n
        return getattr(bpg.ops, t.trace_op)(log_n, to_dev(module.pack_inputs(ops)))

    t = _record(name, module, model, stem, ops_at_2_5=model.edge_ops, model_trace=lambda ops, log_n: model.trace_of(ops),
                device_trace=device_trace, kind_of=lambda family: ALL_ROWS, kinds={ALL_ROWS},
                tuple_of=lambda op, *words: [int(op == o) for o in model.LIVE] + [l for v in words for l in model.limbs(v)],
                **own)
    return t


def _three_lists(model, seed):
    """2^5: fewer rows than a workgroup; 2^7: every edge under every flag, exposed and not; 2^9: two workgroups"""
    return {"edges-2^5": (model.edge_ops, 5), "edges-2^7": (model.edge_ops_full, 7),
            "random-2^9": (lambda: model.random_ops(512, seed), 9)}


def _every_entry(model):
    return tuple(e[0] for e in model.CATALOGUE)


def _division():
    m = arithmetic_div_model

    def answers(op, x, y):
        """(q, r, res) of a live operation, from the statement"""
        q, r = divmod(x, y) if y else (0, x)
        return q, r, 0 if y == 0 else (q if op == m.DIV else r)

    return _row_table(
        "division", arithmetic_div, m, "arithmetic_div", answers=answers, module_ops=(arithmetic_div.OP_DIV, arithmetic_div.OP_MOD),
        model_layout=(m.N_COLS, m.IS_DIV, m.IS_MOD, m.G, m.Z, m.INV, m.X, m.Y, m.RES, m.Q, m.X_BITS, m.Y_BITS, m.Q_BITS,
                      m.R_BITS, m.D_BITS, m.CARRY, m.CARRY_BITS, m.BORROW),
        layout_words=18, in_words=9, wrong_in_words=8, n_cols=1650, width=50, looker_cols=56, n_units=9, n_families=19,
        n_constraints=1686, unpacked=7, exposed_at=3, too_wide=(1, 1 << 256, 1, 0), words_at=5, padding_cells={3: 1},
        witness_lists=_three_lists(m, 0x9D1F), rejected=_every_entry(m), ctl_seed=0xD17C, claim_row=20,
        # rows of the edge list: x / 0, MAX % MAX, MAX / 2, a top-limb y, the largest carry, y = 1
        asked=[1, 7, 8, 12, 17, 2], asked_seed=0xD175)


def _modular():
    m = arithmetic_mod_model

    def answers(op, a, b, mod):
        u = a + b if op == m.ADDMOD else a * b
        q, r = divmod(u, mod) if mod else (u >> 256, u & m.M256)
        return q, r, r if mod else 0

    return _row_table(
        "modular", arithmetic_mod, m, "arithmetic_mod", answers=answers, module_ops=(arithmetic_mod.OP_ADDMOD, arithmetic_mod.OP_MULMOD),
        model_layout=(m.N_COLS, m.IS_ADDMOD, m.IS_MULMOD, m.G, m.Z, m.INV, m.A, m.B_, m.M, m.RES, m.Q, m.A_BITS, m.B_BITS,
                      m.M_BITS, m.Q_BITS, m.R_BITS, m.D_BITS, m.CARRY, m.CARRY_BITS, m.CARRY_OFFSET, m.BORROW),
        layout_words=21, in_words=13, wrong_in_words=9, n_cols=2560, width=66, looker_cols=72, n_units=33, n_families=19,
        n_constraints=2612, unpacked=8, exposed_at=4, too_wide=(1, 1, 1, 1 << 256, 0), words_at=5,
        # z, and the offset 2^20 of each of the 31 signed carries: bit 20 of its 21
        padding_cells={3: 1, **{1893 + 21 * k + 20: 1 for k in range(31)}},
        witness_lists=_three_lists(m, 0x9A0D), rejected=_every_entry(m), ctl_seed=0xA07C, claim_row=21,
        # rows of the edge list: both carry extremes, a product over m = 0, (2^256 - 1)^2 mod 1, a 257-bit q, r = m - 1
        # under either operation, a sum over m = 2^256 - 1
        asked=[0, 1, 3, 5, 10, 12, 13, 8], asked_seed=0xA075)


def _shift():
    m = arithmetic_shift_model
    return _row_table(
        "shift", arithmetic_shift, m, "arithmetic_shift", answers=lambda op, s, x: (m.statement(op, s, x),),
        module_ops=(arithmetic_shift.SHL, arithmetic_shift.SHR, arithmetic_shift.SAR),
        model_layout=(m.N_COLS, m.IS_SHL, m.IS_SHR, m.IS_SAR, m.G, m.Z, m.INV, m.FILL, m.W, m.S, m.X, m.RES, m.Y, m.L, m.E,
                      m.S_BITS, m.X_BITS, m.LO_BITS, m.HI_BITS),
        layout_words=19, in_words=9, wrong_in_words=8, n_cols=1143, width=51, looker_cols=57, n_units=17, n_families=16,
        n_constraints=1165, unpacked=5, exposed_at=3, too_wide=(1, 1 << 256, 1, 0), words_at=8,
        padding_cells={4: 1, 72: 1, 103: 1},                                   # z = [0 < 256], l_0, e at the offset 0
        witness_lists=_three_lists(m, 0x5F1F), rejected=_every_entry(m), ctl_seed=0x5F7C, claim_row=9,
        # rows of the edge list: SHL by 0 and by 16, SHR by 1 and past 256, SAR by 15 and by 0x300, SHL by 2^16 + 5
        asked=[0, 3, 1, 7, 2, 8, 10], asked_seed=0x5F75)


def _signed():
    m = arithmetic_sdiv_model

    def answers(op, x, y):
        """(q, r, res): the quotient and the remainder of the magnitudes, and the result from the statement"""
        ax, ay = abs(signed(x)), abs(signed(y))
        q, r = divmod(ax, ay) if ay else (0, ax)
        return q, r, m.statement(op, x, y)

    return _row_table(
        "signed", arithmetic_sdiv, m, "arithmetic_sdiv", answers=answers, module_ops=(arithmetic_sdiv.OP_SDIV, arithmetic_sdiv.OP_SMOD),
        model_layout=(m.N_COLS, m.IS_SDIV, m.IS_SMOD, m.G, m.Z, m.INV, m.NEG, m.X, m.Y, m.RES, m.Q, m.AY, m.M, m.X_BITS,
                      m.Y_BITS, m.RES_BITS, m.AX_BITS, m.AY_BITS, m.Q_BITS, m.R_BITS, m.D_BITS, m.CARRY, m.CARRY_BITS, m.BORROW,
                      m.X_CHAIN, m.Y_CHAIN, m.RES_CHAIN),
        layout_words=27, in_words=9, wrong_in_words=8, n_cols=2499, width=50, looker_cols=56, n_units=17, n_families=19,
        n_constraints=2583, unpacked=7, exposed_at=3, too_wide=(1, 1 << 256, 1, 0), words_at=6, padding_cells={3: 1},
        # 2^5 rows throughout: this table's rows are the widest of the four
        witness_lists={"edges": (m.edge_ops, 5), "random": (lambda: m.random_ops(32, 0x5D1F), 5)},
        # one wrong witness per family group: the core, the three negations, the sign, the zero test, the flags, the range checks
        rejected=("floor_for_truncation", "remainder_with_the_divisors_sign", "result_with_the_sign_dropped",
                  "negated_result_with_the_last_carry_cleared", "magnitude_not_taken", "magnitude_limb_out_of_range",
                  "remainder_equal_to_the_divisor", "wrap_in_the_high_columns", "no_zero_flag_on_y_zero", "neg_flipped",
                  "both_flags", "exposed_padding_row", "limb_of_two_to_the_16", "remainder_as_quotient", "non_bit_in_res",
                  "non_bit_in_a_carry"),
        ctl_seed=0x5D7C, claim_row=9,
        # rows of the edge list: the quotient 2^255, -2^255 mod 1, x / 0, the truncations under three pairs of signs, the
        # largest carry under both signs of x
        asked=[0, 1, 2, 4, 5, 6, 10, 11], asked_seed=0x5D75)


def _exponentiation():
    """the table whose operations span rows: a list of operations is a trace of a height the caller gives, the inputs are
    pack_ops' (words, starts), the families have kinds, and the tuple is the model's (no flags: one operation)"""
    m = arithmetic_exp_model

    def device_trace(bpg, ops, log_n):
        from util import to_dev
        words, starts = arithmetic_exp.pack_ops(ops, log_n)
        return bpg.ops.arithmetic_exp_trace(log_n, to_dev(words), dev_starts(starts))

    def kind_of(family):
        return TRANSITION if family in m.TRANSITIONS else LAST_ROW if family == "last_row" else ALL_ROWS

    return _record(
        "exponentiation", arithmetic_exp, m, "arithmetic_exp", ops_at_2_5=m.small_ops, model_trace=m.trace_of,
        device_trace=device_trace, kind_of=kind_of, kinds={ALL_ROWS, TRANSITION, LAST_ROW}, tuple_of=m.tuple_of,
        model_layout=(m.N_COLS, m.G, m.FIRST, m.LAST, m.P_, m.E, m.RES, m.R, m.OUT, m.P_BITS, m.R_BITS, m.E_BITS, m.M_BITS,
                      m.S_BITS, m.M_CARRY, m.S_CARRY, m.CARRY_BITS),
        layout_words=17, n_cols=2003, width=48, looker_cols=54, n_units=17, n_families=17, n_constraints=2357, exposed_at=3,
        ctl_seed=0xE87C)


DIVISION, MODULAR, SHIFT, SIGNED, EXPONENTIATION = TABLES = (_division(), _modular(), _shift(), _signed(), _exponentiation())


def _named(*functions):
    return {f.__name__: f for f in functions}


def renamed(tests, **names):
    """`tests` with shared_name=the_files_name applied: a file says "divisions" where the shared body says "the operations" """
    assert set(names) <= set(tests)
    return {names.get(name, name): f for name, f in tests.items()}


# ---------------------------------------------------------------------------------------------- on the CPU
def program_tests(table):
    """The fixtures and the CPU tests every table has: program, reg, the layout entry's refusals, the program's format
    and registration"""
    mod, model = table.module, table.model

    @pytest.fixture(scope="module")
    def program():
        return mod.program()

    @pytest.fixture(scope="module")
    def reg():
        import proof_protocol_decoder_amd as pkg
        pkg.lib()
        return mod.register()

    def test_the_layout_entry_refuses_a_short_or_null_buffer():
        import ctypes as C
        import proof_protocol_decoder_amd as pkg
        entry = getattr(pkg.lib(), table.layout_entry)
        out = (C.c_uint32 * 32)()
        assert entry(out, len(mod.LAYOUT) - 1) == -2
        assert b"%d words" % table.layout_words in pkg.lib().bp_last_error()
        assert entry(out, 0) == -2 and not any(out)
        assert entry(None, 32) == -2
        assert entry(out, 32) == 0 and tuple(out[:len(mod.LAYOUT)]) == mod.LAYOUT

    def test_the_program_fits_the_format_and_registers_once(program, reg):
        import proof_protocol_decoder_amd as pkg
        n_families = table.n_families
        words = program.assemble()
        assert int(words[0]) == int.from_bytes(b"BPGAIRP2", "little")
        assert int(words[7]) <= MAX_REGS and len(program.units) == table.n_units <= 256
        assert len(program.families) == n_families <= MAX_FAMILIES_WITH_PORTS
        assert reg & 0x80000000 and mod.register() == reg and pkg.ops.air_register(words) == reg
        assert pkg.lib().bp_air_count() == 9                                       # no built-in was added
        ids = [t.module.register() for t in TABLES]
        assert reg in ids and len(set(ids)) == len(TABLES)                         # ... and every table keeps its own id
        d = pkg.ops.air_describe(reg)
        assert (d.n_cols, d.degree, d.n_aux, d.n_air_constraints, d.n_units) == (table.n_cols, 3, 2, model.N_CONSTRAINTS, table.n_units)
        fams = [(f.first_index, f.count, f.kind, f.degree) for f in d.families[:d.n_families]]
        first = 0
        for (name, count, *_, degree), got in zip(mod.FAMILIES, fams):
            assert got == (first, count, table.kind_of(name), degree), name
            assert mod.first_index(name) == first
            first += count
        assert {f[2] for f in fams[:n_families]} == table.kinds
        # the library's five constraints of the product port follow the program's own
        assert first == model.N_CONSTRAINTS == table.n_constraints and d.n_families == n_families + 5
        assert sum(f[1] for f in fams[n_families:]) == 5 == d.n_ctl_constraints and fams[n_families][0] == first

    return _named(program, reg, test_the_layout_entry_refuses_a_short_or_null_buffer,
                  test_the_program_fits_the_format_and_registers_once)


def cpu_tests(table):
    """program_tests, and the fixture and the tests the CPU files of the tables of one operation per row have in common:
    edge_trace, the three column maps, the program on every model row, the host checker on the model trace, unpack_row
    and pack_inputs, the catalogue of wrong witnesses"""
    mod, model = table.module, table.model

    @pytest.fixture(scope="module")
    def edge_trace():
        t = model.trace_of(model.edge_ops())
        t.setflags(write=False)
        return t

    def test_the_three_column_maps_agree():
        """the module's constants, the kernel's (its layout entry) and the model's, which is written from AIRS.md"""
        assert mod.kernel_layout() == mod.LAYOUT
        assert table.model_layout == mod.LAYOUT and len(mod.LAYOUT) == table.layout_words
        assert [(n, c) for n, c, _ in mod.FAMILIES] == model.FAMILIES
        assert len(mod.TUPLE_COLS) == table.width and mod.N_COLS == table.n_cols == model.N_COLS
        assert table.module_ops == model.LIVE == tuple(range(1, len(model.LIVE) + 1))

    def test_the_program_vanishes_on_every_model_row(program):
        """every edge under every flag, exposed and not, the padding rows, random operations: 2^7 rows.  The port's
        tuple is the flags and the limb columns from words_at, and on a live row the statement's"""
        for i, op in enumerate(model.edge_ops_full()):
            row = model.cells(model.honest(*op))
            bad = [k for k, v in enumerate(program.evaluate(row, row)) if v]
            assert not bad, (i, op, [model.family_of(k) for k in bad[:4]])
            (f, tup), = program.evaluate_ports(row, row)
            live = op[0] in model.LIVE
            assert f == int(live and bool(op[table.exposed_at])) == row[model.G]
            assert len(tup) == table.width and tup == [row[c] for c in mod.TUPLE_COLS]
            n_flags = len(model.LIVE)
            assert tup == [int(op[0] == o) for o in model.LIVE] + row[table.words_at:table.words_at + table.width - n_flags]
            if live:
                operands = op[1:table.exposed_at]
                assert tup == table.tuple_of(op[0], *operands, table.answers(op[0], *operands)[-1])
            else:   # a padding row, as the kernel writes it
                assert {c: v for c, v in enumerate(row) if v} == table.padding_cells

    def test_the_host_checker_is_clean_on_the_model_trace(reg, edge_trace):
        import proof_protocol_decoder_amd as pkg
        assert edge_trace.shape == (table.n_cols, 32)
        got = pkg.ops.check_air_trace_host(reg, edge_trace)
        assert got.ok and got.n_violations == 0, got

    def test_unpack_row_and_pack_inputs_give_back_the_operations(edge_trace):
        """(op, the operands, what table.answers gives, g) of every row of the edge list, against the statement"""
        ops = model.edge_ops()
        words = mod.pack_inputs(ops)
        assert words.shape == (32, table.in_words) and words.dtype == np.uint64
        for i, (op, *operands, exposed) in enumerate(ops):
            assert int(words[i, 0]) == op | (bool(exposed) << 8)
            for j, v in enumerate(operands):
                assert sum(int(words[i, 1 + 4 * j + k]) << (64 * k) for k in range(4)) == v
            got = mod.unpack_row(edge_trace, i)
            if op not in model.LIVE:
                assert got == (0,) * table.unpacked
                continue
            assert got == (op, *operands, *table.answers(op, *operands), int(bool(exposed))) and len(got) == table.unpacked
        with pytest.raises(ValueError):
            mod.pack_inputs([table.too_wide])

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
        assert {mod.FAMILIES[v.family][0] for v in got.violations} == families
        assert all(model.family_of(v.constraint)[0] == v.family for v in got.violations)

    return dict(program_tests(table), **_named(
        edge_trace, test_the_three_column_maps_agree, test_the_program_vanishes_on_every_model_row,
        test_the_host_checker_is_clean_on_the_model_trace, test_unpack_row_and_pack_inputs_give_back_the_operations,
        test_a_wrong_witness_is_named_at_its_row_and_family))


# ---------------------------------------------------------------------------------------------- on the GPU
def assert_equal_word_for_word(got, want):
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert not len(bad), ("first mismatches (column, row)", bad[:6].tolist(), "of", len(bad))


def proof_tests(table):
    """The mark, the fixtures and the GPU tests every table has: pytestmark, reg, at_2_5 -- the edge list of a table of one
    operation per row, the exponentiation table's small list --, its proof, the port's running products"""
    import air_program_cases as cases
    from util import to_host
    mod, model = table.module, table.model

    @pytest.fixture(scope="module")
    def reg(bpg):
        return mod.register()

    @pytest.fixture(scope="module")
    def at_2_5(bpg):
        """(operations, device trace) of the table's 2^5-row list"""
        ops = table.ops_at_2_5()
        return ops, table.device_trace(bpg, ops, 5)

    def test_the_edge_trace_proves_and_verifies(bpg, reg, at_2_5):
        _, t = at_2_5
        cfg = cases.cfg_for(reg, 5)
        assert (cfg.n_cols, cfg.rate_bits, cfg.deg_pow) == (table.n_cols, 1, 1)
        proof = bpg.ops.stark_prove_trace(reg, cfg, t)
        assert int(proof[4]) == 2 and int(proof[14]) == reg                         # two auxiliary columns: the port's products
        bpg.ops.stark_verify_air(reg, cfg, proof)
        assert cases.verify(7, cases.cfg_for(7, 5), proof) == -5                    # ... under its own id only

    def test_the_ports_running_products_are_the_builders(bpg, reg, at_2_5):
        ops, t = at_2_5
        assert 0 < sum(1 for op in ops if op[0] in model.LIVE and op[table.exposed_at]) < len(ops)
        rng = np.random.default_rng(table.ctl_seed)
        ctl = [int(v) for v in rng.integers(2, model.P, size=4, dtype=np.uint64)]
        got = to_host(bpg.ops.air_port_products(reg, t, ctl))
        want = mod.program().port_running_columns(table.model_trace(ops, 5), ctl)
        assert got.shape == (2, 32) and [[int(v) for v in col] for col in got] == want
        assert int(got[0, 0]) not in (0, 1) and int(got[0, 0]) != int(got[1, 0])

    return dict(pytestmark=pytest.mark.gpu, **_named(reg, at_2_5, test_the_edge_trace_proves_and_verifies,
                                                     test_the_ports_running_products_are_the_builders))


def gpu_tests(table):
    """proof_tests, and the tests the GPU files of the tables of one operation per row have in common: the device witness
    against the model, the kernel's stores, the proof of a wrong witness, a caller's table that looks the operations up,
    the refusals"""
    import air_program_cases as cases
    from air_program_port_cases import LINK, cfg_of
    from util import to_dev, to_host
    mod, model = table.module, table.model
    rejected = [e for e in model.CATALOGUE if e[0] in table.rejected]
    assert len(rejected) == len(table.rejected)

    @pytest.mark.parametrize("which", list(table.witness_lists))
    def test_the_device_witness_is_the_model_and_the_checker_is_clean(bpg, reg, which):
        make, log_n = table.witness_lists[which]
        ops = make()
        assert len(ops) == 1 << log_n
        t = table.device_trace(bpg, ops, log_n)
        assert_equal_word_for_word(to_host(t), model.trace_of(ops))
        got = bpg.ops.check_air_trace(reg, t)
        assert got.ok and got.n_violations == 0, got

    def test_the_kernel_writes_every_cell_and_ignores_what_it_should(bpg):
        """a trace buffer full of ones before the call; bits 9 .. 63 of word 0 and a padding row's operands and exposed bit
        change nothing: a padding row is table.padding_cells and zero elsewhere"""
        import torch
        ops = model.edge_ops()
        words = mod.pack_inputs(ops)
        want = model.trace_of(ops)
        words[:, 0] |= np.uint64(0xABCDEF << 9)
        padding = [i for i, op in enumerate(ops) if op[0] not in model.LIVE]
        assert any(int(words[i, 1:].any()) for i in padding) and any(ops[i][table.exposed_at] for i in padding)   # padding rows carry junk
        out = torch.full((mod.N_COLS, 32), -1, dtype=torch.int64, device="cuda")
        d_words = to_dev(words)
        entry = getattr(bpg.lib(), table.trace_entry)
        assert entry(d_words.data_ptr(), 5, out.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        got = to_host(out)
        assert_equal_word_for_word(got, want)
        for i in padding:
            assert {c: int(got[c, i]) for c in range(mod.N_COLS) if got[c, i]} == table.padding_cells

    @pytest.mark.parametrize("entry", rejected, ids=[e[0] for e in rejected])
    def test_the_proof_of_a_wrong_witness_is_rejected(bpg, reg, at_2_5, entry):
        """the forged row replaces row 9 of the device's edge trace: the device checker names it, the prover proves what it
        is given, the verifier rejects at zeta"""
        _, t = at_2_5
        bad = t.clone()
        bad[:, 9] = to_dev(np.array(model.forged(entry), dtype=np.uint64))
        got = bpg.ops.check_air_trace(reg, bad, max_viol=512)
        assert got.rows == [9] and {mod.FAMILIES[v.family][0] for v in got.violations} == entry[3]
        cfg = cfg_of(reg, 5)
        assert cases.verify(reg, cfg, bpg.ops.stark_prove_trace(reg, cfg, bad)) == -5
        assert b"constraint check at zeta" in bpg.lib().bp_last_error()

    def test_a_callers_table_looks_the_operations_up(bpg, reg):
        """the table exposes the rows table.asked of the edge list and nothing else; the caller claims them in another order"""
        edge_ops = model.edge_ops()
        assert {edge_ops[i][0] for i in table.asked} == set(model.LIVE)
        ops = [o[:-1] + (int(i in table.asked),) for i, o in enumerate(edge_ops)]
        claims = [honest_claim(table, *edge_ops[i]) for i in reversed(table.asked)]
        tables, traces, _ = table_set(bpg, table, reg, ops, claims, table.asked_seed)
        full = with_traces(tables, traces)
        got = bpg.ops.check_table_set(full, LINK)
        n = len(table.asked)
        assert got.ok and got.links[0].holds and (got.links[0].n_looking, got.links[0].n_looked) == (n, n), got
        container = bpg.ops.stark_prove_table_set(full, LINK)
        bpg.ops.stark_verify_table_set(tables, LINK, container)

    def test_refusals(bpg):
        import torch
        from proof_protocol_decoder_amd._lib import BpgError
        trace, w = getattr(bpg.ops, table.trace_op), table.in_words
        good = to_dev(mod.pack_inputs(model.edge_ops()))
        with pytest.raises(BpgError) as e:
            trace(5, None)
        assert e.value.code == -2 and "null inputs" in e.value.message
        with pytest.raises(ValueError, match=r"\[32, %d\]" % w):
            trace(5, good[:31])
        with pytest.raises(ValueError, match=r"\[16, %d\]" % w):
            trace(4, good)
        with pytest.raises(ValueError, match=r"\[32, %d\]" % w):
            trace(5, torch.zeros((32, table.wrong_in_words), dtype=torch.int64, device="cuda"))
        with pytest.raises(ValueError, match="int64"):
            trace(5, good.to(torch.int32))
        with pytest.raises(ValueError, match="device tensors"):
            trace(5, good.cpu())
        # heights outside 4 .. 26 are refused before anything is launched, so the pointers are never read
        entry = getattr(bpg.lib(), table.trace_entry)
        out = torch.zeros(8, dtype=torch.int64, device="cuda")
        for log_n in (3, 27):
            assert entry(good.data_ptr(), log_n, out.data_ptr(), None) == -2
            assert b"log_n out of range" in bpg.lib().bp_last_error()
        assert entry(good.data_ptr(), 5, None, None) == -2
        assert entry(None, 5, out.data_ptr(), None) == -2 and b"null inputs" in bpg.lib().bp_last_error()
        torch.cuda.synchronize()
        assert int(out.sum()) == 0

    return dict(proof_tests(table), **_named(
        test_the_device_witness_is_the_model_and_the_checker_is_clean, test_the_kernel_writes_every_cell_and_ignores_what_it_should,
        test_the_proof_of_a_wrong_witness_is_rejected, test_a_callers_table_looks_the_operations_up, test_refusals))


# ---------------------------------------------------------------------------------------------- table sets
def honest_claim(table, op, *operands_and_exposed):
    operands = operands_and_exposed[:-1]
    return (op, *operands, table.answers(op, *operands)[-1])


def table_set(bpg, table, reg, ops, claims, seed, log_n=5):
    """(statement, [looking trace (numpy), the table's trace (device)], looking rows): a 2^log_n-row table of `ops` and a
    2^4-row table -- pc.flag_program's flag column and the port's tuple -- that sends `claims`, each what table.tuple_of
    takes: (op, operands, res), the exponentiation table's (base, exponent, res)"""
    import air_program_port_cases as pc
    looker = bpg.ops.air_register(pc.flag_program(width=table.width, n_cols=table.looker_cols).assemble())
    rng = np.random.default_rng(seed)
    rows = pc.rows_of(4, rng, len(claims))
    a = pc.flagged(4, rows, [table.tuple_of(*c) for c in claims], rng, width=table.width, n_cols=table.looker_cols)
    tables = [{"air_id": looker, "cfg": pc.cfg_of(looker, 4)}, {"air_id": reg, "cfg": pc.cfg_of(reg, log_n)}]
    return tables, [a, table.device_trace(bpg, ops, log_n)], rows


def one_claim(bpg, table, reg, operation, exposed, res, seed):
    """the table's row table.claim_row (a padding row of the edge list, nothing else exposed) replaced by `operation` =
    (op, operands), the only claim of the looking table, which claims `res` for it; returns (statement, traces, looking row)"""
    ops = [o[:-1] + (0,) for o in table.model.edge_ops()]
    assert ops[table.claim_row][0] not in table.model.LIVE
    ops[table.claim_row] = operation + (exposed,)
    tables, traces, rows = table_set(bpg, table, reg, ops, [operation + (res,)], seed)
    return tables, traces, rows[0]


def with_traces(tables, traces):
    from util import to_dev
    return [dict(tables[0], trace=to_dev(traces[0])), dict(tables[1], trace=traces[1])]


def proves_and_verifies(bpg, tables, traces):
    from air_program_port_cases import LINK
    full = with_traces(tables, traces)
    assert bpg.ops.check_table_set(full, LINK).ok
    bpg.ops.stark_verify_table_set(tables, LINK, bpg.ops.stark_prove_table_set(full, LINK))


def refused_by_the_pre_flight_the_prover_and_the_verifier(bpg, tables, traces, looking_row, looked_row):
    from air_program_port_cases import LINK
    from proof_protocol_decoder_amd._lib import BpgError
    full = with_traces(tables, traces)
    got = bpg.ops.check_table_set(full, LINK)
    assert not got.ok and all(t.ok for t in got.tables) and "link 0 does not balance" in got.message, got.message
    assert "looking row %d (port 0 of table 0)" % looking_row in got.message
    lk, = got.links
    assert not lk.holds and (lk.first_looking_end, lk.first_looking_row, lk.first_looked_row) == (0, looking_row, looked_row), lk
    with pytest.raises(BpgError) as e:
        bpg.ops.stark_prove_table_set(full, LINK)
    assert e.value.code == -5 and "link 0 does not hold" in e.value.message
    container = bpg.ops.stark_prove_table_set(full, LINK, skip_link_check=True)
    with pytest.raises(BpgError) as e:
        bpg.ops.stark_verify_table_set(tables, LINK, container)
    assert e.value.code == -5 and "link 0 does not hold" in e.value.message
