"""Log-derivative lookup ports and range checks on the GPU (csrc/air_program.hip: the LOG forms of
program_port_terms_kernel and quotient_program_kernel; stark_kernels.hip: port_running_columns_kernel; range_mult.hip:
bp_range_multiplicities; the sum identity of a table set's log links).  The reference is Python integers --
Builder.port_running_columns, the fold written here -- and numpy.bincount.  Everything is exact.  CPU side:
tests/test_air_program_log_ports.py."""
import numpy as np
import pytest

import air_program_cases as cases
from air_program_cases import P
from air_program_port_cases import LIMBS, SELF_LINK, cfg_of, count_limbs, range_program, range_witness, self_checked_table
from proof_protocol_decoder_amd._lib import BpgError
from proof_protocol_decoder_amd.air_program import ALL_ROWS, LAST_ROW, TRANSITION, Builder
from test_gpu_air_program import constants_cap
from test_gpu_air_program_ports import challenges, field, members, random_lde
from util import to_dev, to_host

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- 1. the running sums


def mixed_kinds_program():
    """ports of kinds (0, 1, 2, 0) in that order: the columns and the constraint slots of mixed kinds.  Filters: column
    0 (ports 0, 1) and column 4 (ports 2, 3); port 2's tuple reads the next row and the point: the wrap at the last row"""
    b = Builder(8)
    bit = b.family(1, ALL_ROWS, 2)
    b.unit()
    b.emit(bit, b.loc(7) * b.loc(7) - b.loc(7))
    b.port(b.loc(0), [b.loc(1)])
    b.log_port(b.loc(0), [b.loc(1), b.loc(2) + b.loc(3)])
    b.log_port(b.loc(4), [b.nxt(1), b.loc(2) * 3 + b.x], multiplicity=True)
    b.port(b.loc(4), [b.loc(5), b.loc(6)])
    return b


def wide_log_program():
    """a 100-element tuple on a log port: the beta-power table at its full width"""
    b = Builder(104)
    bit = b.family(1, ALL_ROWS, 2)
    b.unit()
    b.emit(bit, b.loc(0) * b.loc(0) - b.loc(0))
    b.log_port(b.loc(0), [b.loc(1 + j) for j in range(100)], multiplicity=True)
    return b


def filter_columns(filters, n, rng):
    """two filter columns: all 0, all 1, mixed bits, or multiplicities -- any field value, p - 1 and values above n among them"""
    if filters == "zero":
        return np.zeros((2, n), np.uint64)
    if filters == "one":
        return np.ones((2, n), np.uint64)
    if filters == "mixed":
        f = rng.integers(0, 2, size=(2, n), dtype=np.uint64)
        f[:, n - 1] = 1                                         # the last row takes part: its nxt is row 0
        return f
    f = field(rng, (2, n))
    f[0, :4], f[1, -4:] = [P - 1, 0, n + 1, 1], [2, P - 1, 3 * n, 0]
    return f


def sums_case(bpg, b, log_n, filters, seed, filter_cols=(0, 4)):
    n = 1 << log_n
    rng = np.random.default_rng(seed)
    t = field(rng, (b.n_cols, n))
    f = filter_columns(filters, n, rng)
    for k, col in enumerate(filter_cols):
        t[col] = f[k]
    ctl = challenges(seed + 1)
    reg = bpg.ops.air_register(b.assemble())
    got = to_host(bpg.ops.air_port_products(reg, to_dev(t), ctl))
    want = b.port_running_columns(t, ctl)
    assert got.shape == (2 * len(b.ports), n)
    for k, col in enumerate(want):
        bad = [i for i, v in enumerate(got[k].tolist()) if v != col[i]]
        assert not bad, ("column", k, "rows", bad[:4], "of", len(bad))
    return got


# 2^5: fewer rows than lanes; 2^10: one partial tile; 2^13: exactly one 8 * 1024 tile; 2^14: two tiles, the carried sum
@pytest.mark.parametrize("filters", ["zero", "one", "mixed", "mult"])
@pytest.mark.parametrize("log_n", [5, 10, 13, 14])
def test_running_sums_of_mixed_kinds_equal_python_integers(bpg, log_n, filters):
    got = sums_case(bpg, mixed_kinds_program(), log_n, filters, 0x1A100 + 16 * log_n)
    if filters == "zero":
        assert bool((got[[0, 1, 6, 7]] == 1).all()) and bool((got[2:6] == 0).all())   # products of ones, sums of zeros
    else:
        assert len(set(got[:, 0].tolist())) == 8


def test_running_sums_of_a_100_element_tuple(bpg):
    sums_case(bpg, wide_log_program(), 10, "mult", 0x1A200, filter_cols=(0,))


# ---------------------------------------------------------------------------------------------- 2. poles


def test_a_pole_contributes_nothing_where_the_filter_is_zero_and_fails_the_call_where_it_is_not(bpg):
    b = mixed_kinds_program()
    reg = bpg.ops.air_register(b.assemble())
    n = 1 << 10
    rng = np.random.default_rng(0x1A300)
    t = field(rng, (8, n))
    t[0], t[4] = rng.integers(0, 2, size=n, dtype=np.uint64), field(rng, n)
    ctl = challenges(0x1A301)
    # port 1: v_0 = t_0 + beta_0 t_1 on row 3; gamma_0 = -v_0 puts a zero of gamma_0 + v_0 there
    v0 = (int(t[1, 3]) + ctl[0] * ((int(t[2, 3]) + int(t[3, 3])) % P)) % P
    ctl[1] = (P - v0) % P
    t[0, 3] = 0
    got = to_host(bpg.ops.air_port_products(reg, to_dev(t), ctl))
    want = b.port_running_columns(t, ctl)
    assert [row.tolist() for row in got] == want
    assert int(got[2, 3]) == int(got[2, 4]) and int(got[3, 3]) == int(got[3, 4])     # the row adds 0 under both sets

    def refused_at_row_3():
        with pytest.raises(BpgError) as e:
            bpg.ops.air_port_products(reg, to_dev(t), ctl)
        assert e.value.code == -5 and "port 1," in e.value.message and "challenge set 0," in e.value.message \
            and "row 3:" in e.value.message, e.value.message
        with pytest.raises(ValueError, match="a pole: port 1, challenge set 0, row 3"):
            b.port_running_columns(t, ctl)

    t[0, 3] = 1
    refused_at_row_3()
    # a second pole in another workgroup's rows does not change the row that is named
    t[1:4, 700], t[0, 700] = t[1:4, 3], 1
    refused_at_row_3()
    # the same table under challenges without a pole is fine again
    assert [row.tolist() for row in to_host(bpg.ops.air_port_products(reg, to_dev(t), challenges(0x1A302)))] == \
        b.port_running_columns(t, challenges(0x1A302))


# ---------------------------------------------------------------------------------------------- 3. K5


def python_quotient(b, log_n, r, loc, nxt, aux, aux_nxt, ctl, alphas, pos):
    """tests/test_gpu_air_program_ports.py's python_quotient with the ports' kinds: a product port's five constraints as
    there; a log port's slot 0 is f f - f (kind 1) or 0 (kind 2), then for c = 0, 1 transition (s_c - s_c') d_c - f, last
    row s_c d_c - f, with s_c = aux column 2 l + c and d_c = gamma_c + sum_j beta_c^j t_j."""
    n = 1 << log_n
    t, m = pos >> log_n, pos & (n - 1)
    inv = lambda v: pow(v % P, P - 2, P)
    x = 7 * pow(pow(7, (P - 1) >> (log_n + r), P), t + (m << r), P) % P
    g = pow(7, (P - 1) >> log_n, P)
    zh = (pow(x, n, P) - 1) % P
    sel = [1, (x - inv(g)) % P, zh * inv(n * (x - 1)) % P, zh * inv(n * (g * x - 1)) % P]
    vals = b.evaluate(loc, nxt, (), (0, 0, 0, 0), x)
    terms = [(i, f[2], vals[i]) for f in b.families for i in range(f[0], f[0] + f[1])]
    T = b.n_constraints + 5 * len(b.ports)
    for l, (f, tup) in enumerate(b.evaluate_ports(loc, nxt, (), (0, 0, 0, 0), x)):
        base, kind = b.n_constraints + 5 * l, b.port_kinds[l]
        terms.append((base, ALL_ROWS, 0 if kind == 2 else (f * f - f) % P))
        for c in range(2):
            d = (ctl[2 * c + 1] + sum(pow(ctl[2 * c], j, P) * tj for j, tj in enumerate(tup))) % P
            z, zn = int(aux[2 * l + c]), int(aux_nxt[2 * l + c])
            if kind == 0:
                term = (1 + f * (d - 1)) % P
                terms.append((base + 1 + 2 * c, TRANSITION, (z - zn * term) % P))
                terms.append((base + 2 + 2 * c, LAST_ROW, (z - term) % P))
            else:
                terms.append((base + 1 + 2 * c, TRANSITION, ((z - zn) * d - f) % P))
                terms.append((base + 2 + 2 * c, LAST_ROW, (z * d - f) % P))
    assert sorted(i for i, _, _ in terms) == list(range(T))
    return [sum(pow(a, T - 1 - i, P) * sel[kind] * v for i, kind, v in terms) * inv(zh) % P for a in alphas]


def three_units_three_kinds():
    """degree 3: a log port's tuple is linear there (s d - f is a last-row constraint)"""
    b = Builder(8)
    bit = b.family(2, ALL_ROWS, 2)
    step = b.family(2, TRANSITION, 3)
    last = b.family(1, LAST_ROW, 2)
    b.unit()
    b.emit(bit, b.loc(0) * b.loc(0) - b.loc(0))
    b.emit(bit + 1, b.loc(4) * b.loc(4) - b.loc(4))
    b.unit()
    b.emit(step, b.nxt(1) - b.loc(1) * b.loc(2) * b.loc(3))
    b.emit(step + 1, b.nxt(2) - b.loc(2) - b.x)
    b.unit()
    b.emit(last, b.loc(5) * b.loc(6) - 7)
    b.port(b.loc(0), [b.loc(1), b.loc(2), b.nxt(3)])
    b.log_port(b.loc(4), [b.loc(5) + 2 * b.loc(6), b.nxt(1)])
    b.log_port(b.loc(4) * b.loc(0), [b.loc(2) + b.x], multiplicity=True)
    return b


def degree_nine_quadratic_tuple():
    b = Builder(8, degree=9)
    deep = b.family(1, ALL_ROWS, 9)
    b.unit()
    v = b.loc(1)
    for k in range(8):
        v = v * b.loc(k % 4)
    b.emit(deep, v - b.loc(7))
    b.log_port(b.loc(0) * b.loc(4), [b.loc(1) * b.loc(2), b.loc(3), b.nxt(5) * b.x])
    b.log_port(b.loc(6), [b.loc(1) * b.loc(1)], multiplicity=True)
    return b


@pytest.mark.parametrize("loaded", [0, 1], ids=["spread", "one-pass"])
@pytest.mark.parametrize("log_n", [5, 9])
@pytest.mark.parametrize("make", [three_units_three_kinds, degree_nine_quadratic_tuple], ids=["deg3-3units-kinds012", "deg9-quadratic-tuple"])
def test_quotient_eval_of_a_program_with_log_ports_equals_the_fold_over_python_integers(bpg, make, log_n, loaded):
    """random LDE and auxiliary matrices (nothing is a valid witness: the fold is compared, not zero), 24 positions: the
    first and the last of every coset the sample holds, and random ones"""
    import torch
    b = make()
    reg = bpg.ops.air_register(b.assemble())
    d = bpg.ops.air_describe(reg)
    deg_pow = 3 if d.degree > 3 else 1
    r = 1 if deg_pow == 1 else 3
    n = 1 << log_n
    rows = n << r
    seed = 0x1B000 + 16 * log_n + d.degree
    lde, aux = random_lde(8, rows, seed), random_lde(d.n_aux, rows, seed + 1)
    assert d.n_aux == 2 * len(b.ports) and d.n_ctl_constraints == 5 * len(b.ports)
    ctl, alphas = challenges(seed + 2), challenges(seed + 3, 2)
    cfg = bpg.ops.stark_cfg(log_n, 8, deg_pow=deg_pow, rate_bits=r)
    with bpg.ops.tuned(assume_loaded=loaded):
        got = bpg.ops.quotient_eval(cfg, lde, aux, None, ctl, alphas, air_id=reg)
    rng = np.random.default_rng(seed + 4)
    pos = [0, n - 1, rows - n, rows - 1, n, 2 * n - 1] + [int(v) for v in rng.integers(0, rows, size=18)]
    nxt = [(p >> log_n) * n + ((p & (n - 1)) + 1) % n for p in pos]
    idx = torch.tensor(pos + nxt, dtype=torch.int64, device="cuda")
    L, A, Q = to_host(lde[:, idx].contiguous()), to_host(aux[:, idx].contiguous()), to_host(got[:, idx[:len(pos)]].contiguous())
    k0 = len(pos)
    for k, p in enumerate(pos):
        want = python_quotient(b, log_n, r, L[:, k], L[:, k0 + k], A[:, k], A[:, k0 + k], ctl, alphas, p)
        assert [int(Q[0, k]), int(Q[1, k])] == want, ("position", p, "coset", p >> log_n, "m", p & (n - 1))


# ---------------------------------------------------------------------------------------------- 4. multiplicities

LDS_LOG = 13    # bp_tune_range_lds_log's default (include/bpg.h): the largest log_range counted in LDS


def wide_values(values, pad=37):
    """the columns as a slice of a wider buffer: stride > n_rows, and what lies between the columns is out of range"""
    import torch
    n_cols, n_rows = values.shape
    wide = torch.full((n_cols, n_rows + pad), -1, dtype=torch.int64, device="cuda")
    wide[:, :n_rows] = to_dev(values)
    return wide[:, :n_rows]


@pytest.mark.parametrize("n_cols", [1, 3])
@pytest.mark.parametrize("log_range", [1, 8, LDS_LOG, LDS_LOG + 1, 20])
def test_range_multiplicities_equal_bincount(bpg, log_range, n_cols):
    """10000 rows: two chunks of rows per column, the last wave of each partial; every third row dropped by the filter
    (and holding values out of range, which nobody looks at); counts added to what d_mult held"""
    n_rows = 10000
    rng = np.random.default_rng(0x1C000 + 4 * log_range + n_cols)
    v = rng.integers(0, 1 << log_range, size=(n_cols, n_rows), dtype=np.uint64)
    v[:, :64] = v[0, 0]                                     # a whole wave of one value
    keep = (np.arange(n_rows) % 3 != 2).astype(np.uint64)
    v[:, keep == 0] = np.uint64(1 << log_range) + v[:, keep == 0]
    before = rng.integers(0, 1 << 40, size=1 << log_range, dtype=np.uint64)
    out = to_dev(before)
    got = bpg.ops.range_multiplicities(wide_values(v), log_range, filter=to_dev(keep), out=out)
    assert got is out
    want = before + np.bincount(v[:, keep == 1].reshape(-1).astype(np.int64), minlength=1 << log_range).astype(np.uint64)
    assert np.array_equal(to_host(got), want)
    # without a filter and into a fresh buffer: every row counts
    inside = v & np.uint64((1 << log_range) - 1)
    assert np.array_equal(to_host(bpg.ops.range_multiplicities(wide_values(inside), log_range)),
                          np.bincount(inside.reshape(-1).astype(np.int64), minlength=1 << log_range).astype(np.uint64))


@pytest.mark.parametrize("log_range", [8, 16])
def test_range_multiplicities_of_one_value_repeated(bpg, log_range):
    """2^16 copies of one value: every lane of every wave on one counter, in LDS and in global memory"""
    import torch
    v = torch.full((1, 1 << 16), 77, dtype=torch.int64, device="cuda")
    got = to_host(bpg.ops.range_multiplicities(v, log_range))
    assert int(got[77]) == 1 << 16 and int(got.sum()) == 1 << 16


def test_range_multiplicities_do_not_depend_on_where_they_are_counted(bpg):
    rng = np.random.default_rng(0x1C100)
    v = to_dev(rng.integers(0, 1 << 10, size=(2, 9000), dtype=np.uint64))
    want = to_host(bpg.ops.range_multiplicities(v, 10))
    try:
        bpg.lib().bp_tune_range_lds_log(9)                  # 2^10 values no longer fit: global atomics
        assert np.array_equal(to_host(bpg.ops.range_multiplicities(v, 10)), want)
    finally:
        bpg.lib().bp_tune_reset()


def test_range_multiplicities_name_the_first_value_out_of_range(bpg):
    log_range, n_rows = 6, 5000
    rng = np.random.default_rng(0x1C200)
    v = rng.integers(0, 1 << log_range, size=(3, n_rows), dtype=np.uint64)
    keep = np.ones(n_rows, dtype=np.uint64)
    keep[[100, 4500]] = 0
    v[0, 100], v[2, 4500] = 1 << log_range, P - 1           # on rows the filter drops: no error
    got = bpg.ops.range_multiplicities(to_dev(v), log_range, filter=to_dev(keep))
    assert np.array_equal(to_host(got), np.bincount(v[:, keep == 1].reshape(-1).astype(np.int64), minlength=64).astype(np.uint64))
    v[1, 4700], v[1, 300], v[2, 7] = P - 1, 1 << log_range, P - 1
    for filt in (None, to_dev(keep)):
        with pytest.raises(BpgError) as e:
            bpg.ops.range_multiplicities(to_dev(v), log_range, filter=filt)
        first = 0 * n_rows + 100 if filt is None else 1 * n_rows + 300
        assert e.value.code == -3 and e.value.first_bad == first, (e.value.message, e.value.first_bad)
        assert "column %d, row %d" % divmod(first, n_rows) in e.value.message
    with pytest.raises(BpgError, match="log_range = 0 is outside 1 .. 24"):
        bpg.ops.range_multiplicities(to_dev(v), 0)


# ---------------------------------------------------------------------------------------------- 5. table sets

def proven(bpg, tables, traces, consts, links, **kw):
    full = [dict(t, trace=to_dev(tr), **({"consts": to_dev(c)} if c is not None else {})) for t, tr, c in zip(tables, traces, consts)]
    return bpg.ops.stark_prove_table_set(full, links, **kw)


def caps_of(bpg, tables, consts):
    return [None if c is None else constants_cap(bpg, to_dev(c), t["cfg"].log_n) for t, c in zip(tables, consts)]


def rejected(bpg, tables, links, container, caps, what):
    with pytest.raises(BpgError) as e:
        bpg.ops.stark_verify_table_set(tables, links, container, const_caps=caps)
    assert e.value.code == -5 and what in e.value.message, e.value.message


def test_a_table_range_checks_its_own_limbs_and_the_constants_are_the_verifiers(bpg):
    reg, t, consts, tables = self_checked_table(bpg)
    assert int(t[4].sum()) == LIMBS * int(t[3].sum()) and bpg.ops.check_air_trace(reg, to_dev(t), consts=to_dev(consts)).ok
    container = proven(bpg, tables, [t], [consts], SELF_LINK)
    caps = caps_of(bpg, tables, [consts])
    bpg.ops.stark_verify_table_set(tables, SELF_LINK, container, const_caps=caps)
    (off, proof), = members(container, SELF_LINK)
    assert int(proof[4]) == 2 * (LIMBS + 1) and int(proof[14]) == reg
    # (e) the statement with the constants cap of another table, 1 .. 64 in place of 0 .. 63
    other = caps_of(bpg, tables, [consts + np.uint64(1)])
    with pytest.raises(BpgError) as e:
        bpg.ops.stark_verify_table_set(tables, SELF_LINK, container, const_caps=other)
    assert e.value.code == -5
    # the kinds are part of the statement: the same shape with the limb ports declared kind 2 is another program
    loose = bpg.ops.air_register(range_program(True).assemble())
    with pytest.raises(BpgError) as e:
        bpg.ops.stark_verify_table_set([{"air_id": loose, "cfg": cfg_of(loose, 6)}], SELF_LINK, container, const_caps=caps)
    assert e.value.code == -5 and "table 0 is proven as" in e.value.message


def test_two_looking_tables_into_one_range_table(bpg):
    """2^5 and 2^7 rows of two 8-bit limbs each into a 2^8-row table; the multiplicities are counted in two calls"""
    looking = bpg.ops.air_register(range_program(n_limbs=2, looked=False).assemble())
    b = Builder(8, n_const=1)
    count = b.family(1, TRANSITION, 1)
    b.unit()
    b.emit(count, b.nxt(5) - b.loc(5) - 1)
    b.log_port(b.loc(4), [b.cst(0)], multiplicity=True)
    looked = bpg.ops.air_register(b.assemble())
    rng = np.random.default_rng(0x1D100)
    a, c = range_witness(5, 256, rng, n_limbs=2), range_witness(7, 256, rng, n_limbs=2)
    mult = count_limbs(bpg, a, 8, n_limbs=2)
    count_limbs(bpg, c, 8, out=mult, n_limbs=2)
    table = np.zeros((8, 256), dtype=np.uint64)
    table[4], table[5] = to_host(mult), np.arange(256, dtype=np.uint64)
    assert int(table[4].sum()) == 2 * int(a[3].sum() + c[3].sum())
    consts = [None, None, np.arange(256, dtype=np.uint64).reshape(1, 256)]
    tables = [{"air_id": looking, "cfg": cfg_of(looking, 5)}, {"air_id": looking, "cfg": cfg_of(looking, 7)},
              {"air_id": looked, "cfg": cfg_of(looked, 8)}]
    links = [([(0, 0), (0, 1), (1, 0), (1, 1)], (2, 0))]
    container = proven(bpg, tables, [a, c, table], consts, links)
    caps = caps_of(bpg, tables, consts)
    bpg.ops.stark_verify_table_set(tables, links, container, const_caps=caps)
    assert [int(p[4]) for _, p in members(container, links)] == [4, 4, 2]
    # one multiplicity too many: the prover's own link check names the link
    table[4, 9] += np.uint64(1)
    with pytest.raises(BpgError) as e:
        proven(bpg, tables, [a, c, table], consts, links)
    assert e.value.code == -5 and "link 0 does not hold" in e.value.message and "port 0 of table 2" in e.value.message


def test_a_limb_out_of_range_is_refused_by_the_prover_and_the_verifier(bpg):
    """(c) one sent limb is 64; the multiplicities are the honest ones of the rest.  The table alone is a valid table --
    its own constraints and its ports' hold -- but no multiplicity column can answer 64: the link does not balance."""
    reg, t, consts, tables = self_checked_table(bpg)
    row = int(np.nonzero(t[3])[0][5])
    t[1, row] = 64
    rest = t[3].copy()
    rest[row] = 0
    mult = bpg.ops.range_multiplicities(to_dev(t)[[0, 2]], 6, filter=to_dev(t[3]))
    t[4] = to_host(bpg.ops.range_multiplicities(to_dev(t)[1:2], 6, filter=to_dev(rest), out=mult))
    with pytest.raises(BpgError) as e:
        count_limbs(bpg, t, 6)
    assert e.value.code == -3 and e.value.first_bad == 1 * 64 + row
    assert bpg.ops.check_air_trace(reg, to_dev(t), consts=to_dev(consts)).ok
    cap, = caps_of(bpg, tables, [consts])
    alone = bpg.ops.stark_prove_trace(reg, tables[0]["cfg"], to_dev(t), consts=to_dev(consts))
    assert cases.verify(reg, tables[0]["cfg"], alone, cap) == 0
    with pytest.raises(BpgError) as e:
        proven(bpg, tables, [t], [consts], SELF_LINK)
    assert e.value.code == -5 and "link 0 does not hold" in e.value.message and "port 3 of table 0" in e.value.message
    container = proven(bpg, tables, [t], [consts], SELF_LINK, skip_link_check=True)
    rejected(bpg, tables, SELF_LINK, container, [cap], "link 0 does not hold")


def test_the_bit_constraint_is_what_makes_membership_sound(bpg):
    """(d) the limb 64 sent twice, with filters 1 and p - 1: the sums over the rows that carry 64 cancel, the link
    balances and the prover's link check passes -- only f f - f, which the library adds to a kind-1 port, sees it.  With
    the limb ports declared kind 2 the same witness is a valid set: multiplicities promise no membership."""
    for limb_kind_multiplicity in (False, True):
        reg, t, consts, tables = self_checked_table(bpg, limb_kind_multiplicity)
        r1, r2 = (int(v) for v in np.nonzero(t[3] == 0)[0][:2])      # two rows that sent nothing
        t[:LIMBS, r1] = t[:LIMBS, r2] = 64
        t[3, r1], t[3, r2] = 1, P - 1
        assert bpg.ops.check_air_trace(reg, to_dev(t), consts=to_dev(consts)).ok    # the checker drops the ports
        container = proven(bpg, tables, [t], [consts], SELF_LINK)        # no BP_SET_SKIP_LINK_CHECK: the link holds
        caps = caps_of(bpg, tables, [consts])
        if limb_kind_multiplicity:
            bpg.ops.stark_verify_table_set(tables, SELF_LINK, container, const_caps=caps)
        else:
            rejected(bpg, tables, SELF_LINK, container, caps, "table 0: constraint check at zeta")
