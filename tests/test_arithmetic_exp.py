"""The exponentiation table on the CPU: the shipped program (proof_protocol_decoder_amd/arithmetic_exp.py) against the
independent model of tests/arithmetic_exp_model.py -- the column maps, Builder.evaluate over Python integers on every row
and next row, the library's host checker -- and a catalogue of wrong witnesses, each named at its row and family.  What
holds for every shipped table -- the layout entry, the program's format and registration, with the kinds of the families
(transition, last row) compared -- is word_tables.program_tests over this table's record; the rest is its own, because
the operations span rows: a forgery is a trace, not a row.  Nothing here needs a GPU; the device side is
tests/test_gpu_arithmetic_exp.py."""
import numpy as np
import pytest

import arithmetic_exp_model as model
from proof_protocol_decoder_amd import arithmetic_div, arithmetic_exp as ex
from word_tables import EXPONENTIATION, program_tests

globals().update(program_tests(EXPONENTIATION))
N_COLS, WIDTH = EXPONENTIATION.n_cols, EXPONENTIATION.width


@pytest.fixture(scope="module")
def small_trace():
    t = model.trace_of(model.small_ops(), 5)
    t.setflags(write=False)
    return t


@pytest.fixture(scope="module")
def edge_traces():
    ts = [model.trace_of(model.edge_ops(), 9), model.trace_of(model.edge_ops_tail(), 9)]
    for t in ts:
        t.setflags(write=False)
    return ts


def builder_violations(program, trace, rows):
    """{(row, family)} by Builder.evaluate over `rows`, the families' kinds applied as the library applies them"""
    n = trace.shape[1]
    out = set()
    for i in rows:
        values = program.evaluate([int(v) for v in trace[:, i]], [int(v) for v in trace[:, (i + 1) % n]])
        out |= {(i, model.family_of(k)[1]) for k, v in enumerate(values) if v and model.applies(model.family_of(k)[1], i, n)}
    return out


def test_the_three_column_maps_agree():
    """the module's constants, the kernel's (its layout entry) and the model's, which is written from AIRS.md"""
    assert ex.kernel_layout() == ex.LAYOUT
    assert EXPONENTIATION.model_layout == ex.LAYOUT and len(ex.LAYOUT) == EXPONENTIATION.layout_words
    assert [(n, c) for n, c, _, _ in ex.FAMILIES] == model.FAMILIES
    assert [k for _, _, k, _ in ex.FAMILIES] == [EXPONENTIATION.kind_of(n) for n, _ in model.FAMILIES]
    assert [ex.first_index(n) for n, _ in model.FAMILIES] == [model.FIRST_INDEX[n] for n, _ in model.FAMILIES]
    assert list(ex.TUPLE_COLS) == model.TUPLE and len(ex.TUPLE_COLS) == WIDTH and ex.N_COLS == N_COLS == model.N_COLS
    assert ex.OP_EXP == model.EXP == 1 and ex.MAX_ROWS == 256
    for e in (0, 1, 2, 3, 255, 256, (1 << 64) + 1, model.M256):
        assert ex.rows_of(e) == model.rows_of(e) == max(1, e.bit_length())


def test_every_unit_cut_states_the_same_constraints(small_trace):
    bad = model.forged(model.CATALOGUE[3])
    rows, nxt = [[int(v) for v in t[:, 0]] for t in (small_trace, bad)], [[int(v) for v in t[:, 1]] for t in (small_trace, bad)]
    honest, want = ex.program().evaluate(rows[0], nxt[0]), ex.program().evaluate(rows[1], nxt[1])
    # Builder.evaluate knows no kinds: row 0 is not the last row, where alone last = 1 is asked for
    assert [k for k, v in enumerate(honest) if v] == [ex.first_index("last_row")] and want != honest
    assert ex.CUTS == (1, 2, 4) and ex.LIMBS_PER_UNIT in ex.CUTS
    for cut in ex.CUTS:
        p = ex.program(cut)
        # a register is 2 KiB of a workgroup's LDS: no cut needs more than 16
        assert len(p.units) == 1 + 16 // cut and int(p.assemble()[7]) <= 16
        assert p.evaluate(rows[0], nxt[0]) == honest and p.evaluate(rows[1], nxt[1]) == want
    with pytest.raises(ValueError):
        ex.program(3)


def test_the_model_rows_state_the_exponentiation():
    """the chains against pow(base, e, 2^256): the first row's tuple, the invariant r p^e on every row, the flags"""
    for ops, log_n in ((model.edge_ops(), 9), (model.edge_ops_tail(), 9), (model.small_ops(), 5), (model.small_ops_to_the_end(), 5)):
        t = model.trace_of(ops, log_n)
        starts = model.first_rows(ops)
        used = starts[-1] + model.rows_of(ops[-1][2])
        for (op, base, e, exposed), at in zip(ops, starts):
            n_rows = model.rows_of(e)
            for i in range(at, at + n_rows):
                first, last, p, rest, res, g = ex.unpack_row(t, i)
                if op != model.EXP:
                    assert [c for c in range(N_COLS) if t[c, i]] == [model.LAST]
                    continue
                r = model.word([int(v) for v in t[model.R:model.R + 16, i]])
                assert (first, last, g) == (int(i == at), int(i == at + n_rows - 1), int(bool(exposed) and i == at))
                assert res == pow(base, e, 1 << 256) == r * pow(p, rest, 1 << 256) % (1 << 256) and rest == e >> (i - at)
                if i == at:
                    assert (p, rest) == (base, e) and [int(t[c, i]) for c in ex.TUPLE_COLS] == model.tuple_of(base, e, res)
        for i in range(used, 1 << log_n):
            assert [c for c in range(N_COLS) if t[c, i]] == [model.LAST]
    assert pow(0, 0, 1 << 256) == 1 == ex.unpack_row(model.trace_of([(1, 0, 0, 1)], 4), 0)[4]      # 0^0 = 1
    assert ex.unpack_row(model.trace_of([(1, 2, 256, 1)], 4), 0)[4] == 0                          # not 2^(256 mod 256)
    assert ex.unpack_row(model.trace_of([(1, 3, model.SIXTY_FOUR, 1)], 7), 0)[4] == pow(3, (1 << 64) + 1, 1 << 256) != 3


def test_the_edge_lists_cover_what_the_statement_singles_out():
    ops = model.edge_ops()
    M = model.M256
    assert sum(model.rows_of(o[2]) for o in ops) == 512                        # the last operation ends on the last row
    assert ops[-1][0] == model.EXP and model.rows_of(ops[-1][2]) > 1
    live = {(o[1], o[2]) for o in ops if o[0] == model.EXP}
    assert {(0, 0), (0, 1), (1, M), (M, 2), (2, 255), (2, 256), (3, (1 << 64) + 1), (model.ONES, 3)} <= live
    assert any(model.rows_of(o[2]) == 256 for o in ops)                        # one full operation
    assert any(o[0] == model.EXP and not o[3] for o in ops) and any(o[0] != model.EXP and o[1] and o[3] for o in ops)
    assert model.edge_ops_tail() == [(model.EXP, M, M, 1)]                     # ... and every row of this one multiplies
    assert model.first_rows(model.small_ops()) == model.SMALL_STARTS
    assert sum(model.rows_of(o[2]) for o in model.small_ops()) == 28 and sum(model.rows_of(o[2]) for o in model.small_ops_to_the_end()) == 32


def test_the_largest_values_are_below_the_field(edge_traces):
    """AIRS.md: a product column stays below 2^37; the largest carry, 0xFFFEF out of column 15 of (2^256 - 1)^2, needs all
    20 bits"""
    assert 16 * 0xFFFF * 0xFFFF + (1 << 20) < 1 << 37 < model.P
    ones = model.limbs(model.ONES)
    cs = model.carries(ones, ones, model.limbs(model.ONES * model.ONES & model.M256))
    assert max(cs) == cs[15] == model.LARGEST_CARRY and model.LARGEST_CARRY >> 19 == 1
    largest = 0
    for t in edge_traces:
        for col in (model.M_CARRY, model.S_CARRY):
            for k in range(16):
                bits = t[col + 20 * k:col + 20 * k + 20, :].astype(object)
                largest = max(largest, max(sum(int(b) << j for j, b in enumerate(bits[:, i])) for i in range(t.shape[1])))
    assert largest == model.LARGEST_CARRY


def test_the_program_vanishes_on_every_row_and_next_row_of_the_model_traces(program, edge_traces, small_trace):
    """Builder.evaluate over Python integers on the 2^5-row trace and on 2^9 rows of edges, every row with its next row
    (the last row's is row 0, as the prover has it); the model's own statement of the constraints agrees; the port's filter
    and tuple are the model's"""
    for t in [small_trace, model.trace_of(model.small_ops_to_the_end(), 5)] + edge_traces:
        n = t.shape[1]
        rows = range(n)
        assert builder_violations(program, t, rows) == set()
        assert model.violations(t, rows) == []
        for i in rows:
            (f, tup), = program.evaluate_ports([int(v) for v in t[:, i]], [int(v) for v in t[:, (i + 1) % n]])
            assert f == int(t[model.G, i]) and tup == [int(t[c, i]) for c in model.TUPLE] and len(tup) == WIDTH


def test_the_host_checker_is_clean_on_the_model_traces(reg, edge_traces, small_trace):
    import proof_protocol_decoder_amd as pkg
    for t in [small_trace, model.trace_of(model.small_ops_to_the_end(), 5)] + edge_traces:
        got = pkg.ops.check_air_trace_host(reg, np.ascontiguousarray(t))
        assert got.ok and got.n_violations == 0, got


def test_pack_ops_and_unpack_row_give_back_the_operations(small_trace):
    ops = model.small_ops()
    words, starts = ex.pack_ops(ops, 5)
    assert words.shape == (8, 9) and words.dtype == np.uint64 and starts.dtype == np.uint32
    assert [int(v) for v in starts] == model.SMALL_STARTS + [28]
    assert (words == arithmetic_div.pack_inputs(ops)).all()                    # the division table's input words
    for (op, base, e, exposed), at in zip(ops, model.SMALL_STARTS):
        got = ex.unpack_row(small_trace, at)
        assert got == ((1, int(e < 2), base, e, pow(base, e, 1 << 256), int(bool(exposed))) if op == model.EXP else (0, 1, 0, 0, 0, 0))
    assert [int(v) for v in ex.pack_ops(model.small_ops_to_the_end(), 5)[1]][-1] == 32
    with pytest.raises(ValueError, match="ends at row 33"):
        ex.pack_ops(model.small_ops_to_the_end() + [(1, 2, 0, 0)], 5)
    with pytest.raises(ValueError, match="ends at row 17"):
        ex.pack_ops([(1, 2, 1 << 16, 0)], 4)
    with pytest.raises(ValueError):
        ex.pack_ops([(1, 1 << 256, 1, 0)], 5)
    words, starts = ex.pack_ops([], 5)
    assert words.shape == (0, 9) and [int(v) for v in starts] == [0]


def test_the_catalogue_breaks_every_family():
    assert {f for e in model.CATALOGUE for _, f in e[2]} == {name for name, _ in model.FAMILIES}
    assert len({e[0] for e in model.CATALOGUE}) == len(model.CATALOGUE)
    # every entry changes the trace; eleven rewrite two to four rows -- a chain kept consistent after the forged step -- and
    # each of those is still expected at one row: the rest of what it rewrites must stand
    honest = model.trace_of(model.small_ops(), 5)
    rewritten = {e[0]: int((model.forged(e) != honest).any(axis=0).sum()) for e in model.CATALOGUE}
    assert all(rewritten.values()) and sorted(k for k in rewritten.values() if k > 1) == [2, 2, 3, 3, 3, 3, 3, 3, 3, 3, 4]
    assert all(len({row for row, _ in e[2]}) == 1 for e in model.CATALOGUE if rewritten[e[0]] > 1)


@pytest.mark.parametrize("entry", model.CATALOGUE, ids=[e[0] for e in model.CATALOGUE])
def test_a_wrong_witness_is_named_at_its_row_and_family(program, reg, entry):
    """the forgery rewrites rows of the 2^5-row trace; the model's statement of the constraints, Builder.evaluate and the
    host checker name the same constraints at the same rows, all of them where the forgery means to break"""
    import proof_protocol_decoder_amd as pkg
    name, _, expected = entry
    t = model.forged(entry)
    named = model.violations(t)
    assert named and {(row, family) for row, family, _ in named} == expected, (name, named[:8])
    assert builder_violations(program, t, range(32)) == expected
    got = pkg.ops.check_air_trace_host(reg, t, max_viol=512)
    assert got.rows == sorted({row for row, _ in expected}) and got.n_violations == len(named)
    assert sorted((v.row, v.constraint) for v in got.violations) == sorted((row, k) for row, _, k in named)
    assert {(v.row, ex.FAMILIES[v.family][0]) for v in got.violations} == expected
    assert all(model.family_of(v.constraint)[0] == v.family for v in got.violations)
