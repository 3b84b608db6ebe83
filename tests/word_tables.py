"""What the tests know about the shipped tables over 256-bit words -- the division table and the modular table --, stated
once.  A plain module, not collected, in the manner of tests/builtin_airs.py.

DIVISION and MODULAR are one record per table: the package module, the independent row model, the entry names, the
input words, and as literals the shapes AIRS.md section 2 states (columns, port width, units, constraints), the seeds
and the rows its table-set scenario asks for.  Below them: the fixtures and bodies tests/test_arithmetic_{div,mod}.py
have in common (cpu_tests) and those of tests/test_gpu_arithmetic_{div,mod}.py (gpu_tests), which those files bind to
their own test names; and the helpers of the table-set stories each GPU file tells for itself."""
from types import SimpleNamespace

import numpy as np
import pytest

import arithmetic_div_model
import arithmetic_mod_model
from proof_protocol_decoder_amd import arithmetic_div, arithmetic_mod
from proof_protocol_decoder_amd.air_program import MAX_FAMILIES_WITH_PORTS, MAX_REGS


def _division():
    m = arithmetic_div_model

    def answers(op, x, y):
        """(q, r, res) of a live operation, from the statement"""
        q, r = divmod(x, y) if y else (0, x)
        return q, r, 0 if y == 0 else (q if op == m.DIV else r)

    return SimpleNamespace(
        name="division", module=arithmetic_div, model=m, answers=answers,
        layout_entry="bp_arithmetic_div_layout", trace_entry="bp_arithmetic_div_trace", trace_op="arithmetic_div_trace",
        model_layout=(m.N_COLS, m.IS_DIV, m.IS_MOD, m.G, m.Z, m.INV, m.X, m.Y, m.RES, m.Q, m.X_BITS, m.Y_BITS, m.Q_BITS,
                      m.R_BITS, m.D_BITS, m.CARRY, m.CARRY_BITS, m.BORROW),
        layout_words=18, in_words=9, wrong_in_words=8, n_cols=1650, width=50, looker_cols=56, n_units=9, n_constraints=1686,
        exposed_at=3, too_wide=(1, 1 << 256, 1, 0), random_seed=0x9D1F, ctl_seed=0xD17C,
        # rows of the edge list: x / 0, MAX % MAX, MAX / 2, a top-limb y, the largest carry, y = 1
        asked=[1, 7, 8, 12, 17, 2], asked_seed=0xD175)


def _modular():
    m = arithmetic_mod_model

    def answers(op, a, b, mod):
        u = a + b if op == m.ADDMOD else a * b
        q, r = divmod(u, mod) if mod else (u >> 256, u & m.M256)
        return q, r, r if mod else 0

    return SimpleNamespace(
        name="modular", module=arithmetic_mod, model=m, answers=answers,
        layout_entry="bp_arithmetic_mod_layout", trace_entry="bp_arithmetic_mod_trace", trace_op="arithmetic_mod_trace",
        model_layout=(m.N_COLS, m.IS_ADDMOD, m.IS_MULMOD, m.G, m.Z, m.INV, m.A, m.B_, m.M, m.RES, m.Q, m.A_BITS, m.B_BITS,
                      m.M_BITS, m.Q_BITS, m.R_BITS, m.D_BITS, m.CARRY, m.CARRY_BITS, m.CARRY_OFFSET, m.BORROW),
        layout_words=21, in_words=13, wrong_in_words=9, n_cols=2560, width=66, looker_cols=72, n_units=33, n_constraints=2612,
        exposed_at=4, too_wide=(1, 1, 1, 1 << 256, 0), random_seed=0x9A0D, ctl_seed=0xA07C,
        # rows of the edge list: both carry extremes, a product over m = 0, (2^256 - 1)^2 mod 1, a 257-bit q, r = m - 1
        # under either operation, a sum over m = 2^256 - 1
        asked=[0, 1, 3, 5, 10, 12, 13, 8], asked_seed=0xA075)


DIVISION, MODULAR = _division(), _modular()
LIVE = (1, 2)   # the op bytes of a table's two operations; any other is a padding row


# ---------------------------------------------------------------------------------------------- on the CPU
def cpu_tests(table):
    """The fixtures and the tests the two CPU files have in common:
        program, reg, edge_trace, test_the_three_column_maps_agree, <the layout entry's refusals>,
            test_the_program_fits_the_format_and_registers_once, test_the_program_vanishes_on_every_model_row,
            test_the_host_checker_is_clean_on_the_model_trace, <unpack_row and pack_inputs>,
            test_a_wrong_witness_is_named_at_its_row_and_family = cpu_tests(table)"""
    mod, model = table.module, table.model

    @pytest.fixture(scope="module")
    def program():
        return mod.program()

    @pytest.fixture(scope="module")
    def reg():
        import proof_protocol_decoder_amd as pkg
        pkg.lib()
        return mod.register()

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
        words = program.assemble()
        assert int(words[0]) == int.from_bytes(b"BPGAIRP2", "little")
        assert int(words[7]) <= MAX_REGS and len(program.units) == table.n_units <= 256
        assert len(program.families) == 19 <= MAX_FAMILIES_WITH_PORTS
        assert reg & 0x80000000 and mod.register() == reg and pkg.ops.air_register(words) == reg
        assert pkg.lib().bp_air_count() == 9                                       # no built-in was added
        other = MODULAR if table is DIVISION else DIVISION
        assert other.module.register() != reg                                      # ... and the other table keeps its own id
        d = pkg.ops.air_describe(reg)
        assert (d.n_cols, d.degree, d.n_aux, d.n_air_constraints, d.n_units) == (table.n_cols, 3, 2, model.N_CONSTRAINTS, table.n_units)
        fams = [(f.first_index, f.count, f.kind, f.degree) for f in d.families[:d.n_families]]
        first = 0
        for (name, count, degree), got in zip(mod.FAMILIES, fams):
            assert got == (first, count, 0, degree), name
            assert mod.first_index(name) == first
            first += count
        # the library's five constraints of the product port follow the program's own
        assert first == model.N_CONSTRAINTS == table.n_constraints and d.n_families == 19 + 5
        assert sum(f[1] for f in fams[19:]) == 5 == d.n_ctl_constraints and fams[19][0] == first

    def test_the_program_vanishes_on_every_model_row(program):
        """every edge under both flags, exposed and not, the padding rows, random operations: 2^7 rows"""
        for i, op in enumerate(model.edge_ops_full()):
            row = model.cells(model.honest(*op))
            bad = [k for k, v in enumerate(program.evaluate(row, row)) if v]
            assert not bad, (i, op, [model.family_of(k) for k in bad[:4]])
            (f, tup), = program.evaluate_ports(row, row)
            want_g = int(op[0] in LIVE and bool(op[table.exposed_at]))
            assert f == want_g and len(tup) == table.width and tup == [row[c] for c in mod.TUPLE_COLS]

    def test_the_host_checker_is_clean_on_the_model_trace(reg, edge_trace):
        import proof_protocol_decoder_amd as pkg
        assert edge_trace.shape == (table.n_cols, 32)
        got = pkg.ops.check_air_trace_host(reg, edge_trace)
        assert got.ok and got.n_violations == 0, got

    def test_unpack_row_and_pack_inputs_give_back_the_operations(edge_trace):
        """(op, the operands, q, r, res, g) of every row of the edge list, against the statement"""
        ops = model.edge_ops()
        words = mod.pack_inputs(ops)
        assert words.shape == (32, table.in_words) and words.dtype == np.uint64
        for i, (op, *operands, exposed) in enumerate(ops):
            assert int(words[i, 0]) == op | (bool(exposed) << 8)
            for j, v in enumerate(operands):
                assert sum(int(words[i, 1 + 4 * j + k]) << (64 * k) for k in range(4)) == v
            got = mod.unpack_row(edge_trace, i)
            if op not in LIVE:
                assert got == (0,) * (len(operands) + 5)
                continue
            assert got == (op, *operands, *table.answers(op, *operands), int(bool(exposed)))
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

    return (program, reg, edge_trace, test_the_three_column_maps_agree, test_the_layout_entry_refuses_a_short_or_null_buffer,
            test_the_program_fits_the_format_and_registers_once, test_the_program_vanishes_on_every_model_row,
            test_the_host_checker_is_clean_on_the_model_trace, test_unpack_row_and_pack_inputs_give_back_the_operations,
            test_a_wrong_witness_is_named_at_its_row_and_family)


# ---------------------------------------------------------------------------------------------- on the GPU
def device_trace(bpg, table, ops):
    from util import to_dev
    log_n = len(ops).bit_length() - 1
    return getattr(bpg.ops, table.trace_op)(log_n, to_dev(table.module.pack_inputs(ops)))


def assert_equal_word_for_word(got, want):
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert not len(bad), ("first mismatches (column, row)", bad[:6].tolist(), "of", len(bad))


def tuple_of(table, op, *operands_and_result):
    """the port's tuple: the two flags, then the limbs of every operand and of the result"""
    return [int(op == 1), int(op == 2)] + [l for v in operands_and_result for l in table.model.limbs(v)]


def honest_claim(table, op, *operands_and_exposed):
    operands = operands_and_exposed[:-1]
    return (op, *operands, table.answers(op, *operands)[2])


def table_set(bpg, table, reg, ops, claims, seed):
    """(statement, [looking trace (numpy), the table's trace (device)], looking rows): a 2^5-row table of `ops` and a
    2^4-row table -- pc.flag_program's flag column and the port's tuple -- that sends `claims` = [(op, operands, res), ...]"""
    import air_program_port_cases as pc
    looker = bpg.ops.air_register(pc.flag_program(width=table.width, n_cols=table.looker_cols).assemble())
    rng = np.random.default_rng(seed)
    rows = pc.rows_of(4, rng, len(claims))
    a = pc.flagged(4, rows, [tuple_of(table, *c) for c in claims], rng, width=table.width, n_cols=table.looker_cols)
    tables = [{"air_id": looker, "cfg": pc.cfg_of(looker, 4)}, {"air_id": reg, "cfg": pc.cfg_of(reg, 5)}]
    return tables, [a, device_trace(bpg, table, ops)], rows


def one_claim(bpg, table, reg, row, operation, exposed, res, seed):
    """the table's row `row` (a padding row of the edge list, nothing else exposed) replaced by `operation` = (op,
    operands), the only claim of the looking table, which claims `res` for it; returns (statement, traces, looking row)"""
    ops = [o[:-1] + (0,) for o in table.model.edge_ops()]
    assert ops[row][0] not in LIVE
    ops[row] = operation + (exposed,)
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


def gpu_tests(table):
    """The fixtures and the tests the two GPU files have in common:
        pytestmark, reg, edge, test_the_device_witness_is_the_model_and_the_checker_is_clean,
            test_the_kernel_writes_every_cell_and_ignores_what_it_should, test_the_edge_trace_proves_and_verifies,
            test_the_proof_of_a_wrong_witness_is_rejected, test_the_ports_running_products_are_the_builders,
            <a caller's table looks the operations up>, test_refusals = gpu_tests(table)"""
    import air_program_cases as cases
    from air_program_port_cases import LINK, cfg_of
    from util import to_dev, to_host
    mod, model = table.module, table.model

    @pytest.fixture(scope="module")
    def reg(bpg):
        return mod.register()

    @pytest.fixture(scope="module")
    def edge(bpg):
        """(operations, device trace) of the 2^5-row edge list"""
        ops = model.edge_ops()
        return ops, device_trace(bpg, table, ops)

    # 2^5: fewer rows than a workgroup; 2^7: every edge under both flags, exposed and not; 2^9: two workgroups
    @pytest.mark.parametrize("which", ["edges-2^5", "edges-2^7", "random-2^9"])
    def test_the_device_witness_is_the_model_and_the_checker_is_clean(bpg, reg, which):
        ops = {"edges-2^5": model.edge_ops, "edges-2^7": model.edge_ops_full,
               "random-2^9": lambda: model.random_ops(512, table.random_seed)}[which]()
        t = device_trace(bpg, table, ops)
        assert_equal_word_for_word(to_host(t), model.trace_of(ops))
        got = bpg.ops.check_air_trace(reg, t)
        assert got.ok and got.n_violations == 0, got

    def test_the_kernel_writes_every_cell_and_ignores_what_it_should(bpg):
        """a trace buffer full of ones before the call; bits 9 .. 63 of word 0 and a padding row's operands change nothing"""
        import torch
        ops = model.edge_ops()
        words = mod.pack_inputs(ops)
        want = model.trace_of(ops)
        words[:, 0] |= np.uint64(0xABCDEF << 9)
        assert any(int(words[i, 1:].any()) for i, op in enumerate(ops) if op[0] not in LIVE)   # padding rows carry junk
        out = torch.full((mod.N_COLS, 32), -1, dtype=torch.int64, device="cuda")
        d_words = to_dev(words)
        entry = getattr(bpg.lib(), table.trace_entry)
        assert entry(d_words.data_ptr(), 5, out.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        assert_equal_word_for_word(to_host(out), want)

    def test_the_edge_trace_proves_and_verifies(bpg, reg, edge):
        _, t = edge
        cfg = cases.cfg_for(reg, 5)
        assert (cfg.n_cols, cfg.rate_bits, cfg.deg_pow) == (table.n_cols, 1, 1)
        proof = bpg.ops.stark_prove_trace(reg, cfg, t)
        assert int(proof[4]) == 2 and int(proof[14]) == reg                         # two auxiliary columns: the port's products
        bpg.ops.stark_verify_air(reg, cfg, proof)
        assert cases.verify(7, cases.cfg_for(7, 5), proof) == -5                    # ... under its own id only

    @pytest.mark.parametrize("entry", model.CATALOGUE, ids=[e[0] for e in model.CATALOGUE])
    def test_the_proof_of_a_wrong_witness_is_rejected(bpg, reg, edge, entry):
        """the forged row replaces row 9 of the device's edge trace: the device checker names it, the prover proves what it
        is given, the verifier rejects at zeta"""
        _, t = edge
        bad = t.clone()
        bad[:, 9] = to_dev(np.array(model.forged(entry), dtype=np.uint64))
        got = bpg.ops.check_air_trace(reg, bad, max_viol=512)
        assert got.rows == [9] and {mod.FAMILIES[v.family][0] for v in got.violations} == entry[3]
        cfg = cfg_of(reg, 5)
        assert cases.verify(reg, cfg, bpg.ops.stark_prove_trace(reg, cfg, bad)) == -5
        assert b"constraint check at zeta" in bpg.lib().bp_last_error()

    def test_the_ports_running_products_are_the_builders(bpg, reg, edge):
        ops, t = edge
        assert 0 < sum(1 for op in ops if op[0] in LIVE and op[table.exposed_at]) < 32
        rng = np.random.default_rng(table.ctl_seed)
        ctl = [int(v) for v in rng.integers(2, model.P, size=4, dtype=np.uint64)]
        got = to_host(bpg.ops.air_port_products(reg, t, ctl))
        want = mod.program().port_running_columns(model.trace_of(ops), ctl)
        assert got.shape == (2, 32) and [[int(v) for v in col] for col in got] == want
        assert int(got[0, 0]) not in (0, 1) and int(got[0, 0]) != int(got[1, 0])

    def test_a_callers_table_looks_the_operations_up(bpg, reg):
        """the table exposes the rows table.asked of the edge list and nothing else; the caller claims them in another order"""
        edge_ops = model.edge_ops()
        assert {edge_ops[i][0] for i in table.asked} == set(LIVE)
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
        torch.cuda.synchronize()
        assert int(out.sum()) == 0

    return (pytest.mark.gpu, reg, edge, test_the_device_witness_is_the_model_and_the_checker_is_clean,
            test_the_kernel_writes_every_cell_and_ignores_what_it_should, test_the_edge_trace_proves_and_verifies,
            test_the_proof_of_a_wrong_witness_is_rejected, test_the_ports_running_products_are_the_builders,
            test_a_callers_table_looks_the_operations_up, test_refusals)
