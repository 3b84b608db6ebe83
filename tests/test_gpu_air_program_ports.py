"""Lookup ports of run-time AIRs and table sets on the GPU (csrc/air_program.hip: program_port_terms_kernel and the port
units of quotient_program_kernel; bp_air_port_products, bp_stark_prove_table_set, bp_stark_verify_table_set).  The
reference is Python integers -- Builder.evaluate_ports and the products / the fold written in
tests/air_program_port_cases.py and here -- and the built-in AIR 3 kernels.  Everything is exact.  CPU side:
tests/test_air_program_ports.py."""
import numpy as np
import pytest

import air_program_cases as cases
import air_program_port_cases as pc
from air_program_cases import P
from air_program_port_cases import LINK, WIDTH, balanced_pair, cfg_of, field, flagged, rows_of
from proof_protocol_decoder_amd.air_program import ALL_ROWS, LAST_ROW, TRANSITION, Builder
from util import to_dev, to_host

pytestmark = pytest.mark.gpu


def random_lde(n_cols, rows, seed):
    """uniform words below 2^63 (canonical), the field's edge values sprinkled in, made on the device"""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    m = torch.randint(0, 2 ** 63 - 1, (n_cols, rows), dtype=torch.int64, device="cuda", generator=g)
    flat = m.view(-1)
    for k, v in enumerate([0, 1, P - 1, 0xFFFFFFFF, 1 << 32, P - (1 << 32), 0xFFFFFFFF00000000, 2]):
        flat[(k * 7919) % flat.numel()] = v - (1 << 64) if v >= 1 << 63 else v
    return m


def challenges(seed, k=4):
    rng = np.random.default_rng(seed)
    return [int(v) for v in rng.integers(2, P, size=k, dtype=np.uint64)]


# ---------------------------------------------------------------------------------------------- 1. the products


def two_port_program(n_cols=8):
    """tuple lengths 1 and 3; the second filter is another column, its middle element a sum"""
    b = Builder(n_cols)
    bit = b.family(2, ALL_ROWS, 2)
    b.unit()
    f0, f1 = b.loc(0), b.loc(4)
    b.emit(bit, f0 * f0 - f0)
    b.emit(bit + 1, f1 * f1 - f1)
    b.port(f0, [b.loc(1)])
    b.port(f1, [b.loc(1), b.loc(2) + b.loc(3), b.loc(5)])
    return b


def wide_program():
    """a 100-element tuple: the beta-power table at keccak_sponge -> keccak_f's width"""
    b = Builder(104)
    bit = b.family(1, ALL_ROWS, 2)
    b.unit()
    b.emit(bit, b.loc(0) * b.loc(0) - b.loc(0))
    b.port(b.loc(0), [b.loc(1 + j) for j in range(100)])
    return b


def wrap_program():
    """a filter that is a sum of two columns and a tuple element that reads the next row: the wrap at the last row"""
    b = Builder(8)
    bit = b.family(1, ALL_ROWS, 2)
    b.unit()
    b.emit(bit, b.loc(0) * b.loc(0) - b.loc(0))
    b.port(b.loc(0) + b.loc(4), [b.nxt(1), b.loc(2) * 3 + b.x])
    return b


def product_case(bpg, b, log_n, filters, seed):
    n = 1 << log_n
    rng = np.random.default_rng(seed)
    t = field(rng, (b.n_cols, n))
    for col in (0, 4):
        t[col] = {"zero": np.zeros(n, np.uint64), "one": np.ones(n, np.uint64),
                  "mixed": rng.integers(0, 2, size=n, dtype=np.uint64)}[filters]
    if filters == "mixed":
        t[0, n - 1] = 1                                         # the last row takes part: its nxt is row 0
    ctl = challenges(seed + 1)
    reg = bpg.ops.air_register(b.assemble())
    got = to_host(bpg.ops.air_port_products(reg, to_dev(t), ctl))
    want = pc.port_products(b, t, ctl)
    assert got.shape == (2 * len(b.ports), n)
    for k, col in enumerate(want):
        bad = [i for i in range(n) if int(got[k, i]) != col[i]]
        assert not bad, ("column", k, "rows", bad[:4], "of", len(bad))
    return got


# 2^5: fewer rows than lanes; 2^10: one element per lane; 2^13: exactly one full tile; 2^14: two tiles, the carried product
@pytest.mark.parametrize("filters", ["zero", "one", "mixed"])
@pytest.mark.parametrize("log_n", [5, 10, 13, 14])
def test_port_products_equal_the_products_over_python_integers(bpg, log_n, filters):
    got = product_case(bpg, two_port_program(), log_n, filters, 0xA100 + log_n)
    if filters == "zero":
        assert bool((got == 1).all())                           # every term is 1
    else:
        assert len(set(got[:, 0].tolist())) == 4


def test_port_products_of_a_100_element_tuple(bpg):
    product_case(bpg, wide_program(), 10, "mixed", 0xA200)


def test_port_products_wrap_at_the_last_row(bpg):
    """the filter is loc(0) + loc(4) (0, 1 or 2 here: the product does not ask for a bit) and t_0 = nxt(1)"""
    b = wrap_program()
    got = product_case(bpg, b, 10, "mixed", 0xA300)
    # the last row's term reads row 0: changing t[1, 0] changes z at the last row
    n = 1 << 10
    rng = np.random.default_rng(0xA300)
    t = field(rng, (8, n))
    t[0], t[4] = 1, 0
    ctl = challenges(0xA301)
    reg = bpg.ops.air_register(b.assemble())
    a = to_host(bpg.ops.air_port_products(reg, to_dev(t), ctl))
    t[1, 0] = (int(t[1, 0]) + 1) % P
    c = to_host(bpg.ops.air_port_products(reg, to_dev(t), ctl))
    assert int(a[0, n - 1]) != int(c[0, n - 1]) and int(c[0, n - 1]) == pc.port_products(b, t, ctl)[0][n - 1]
    assert got.shape == (2, n)


def test_port_products_of_a_column_slice_and_refusals(bpg):
    import torch
    from proof_protocol_decoder_amd._lib import BpgError
    b = two_port_program()
    reg = bpg.ops.air_register(b.assemble())
    rng = np.random.default_rng(0xA400)
    t = field(rng, (8, 64))
    t[0], t[4] = rng.integers(0, 2, size=64, dtype=np.uint64), 1
    ctl = challenges(0xA401)
    wide = torch.zeros((8, 3 * 64), dtype=torch.int64, device="cuda")
    wide[:, :64] = to_dev(t)
    assert bool((bpg.ops.air_port_products(reg, wide[:, :64], ctl) == bpg.ops.air_port_products(reg, to_dev(t), ctl)).all())
    with pytest.raises(BpgError, match="no registered program with lookup ports"):
        bpg.ops.air_port_products(cases.register(cases.memory_program()), bpg.ops.memory_trace(5, seed=1), ctl)
    with pytest.raises(BpgError, match="no registered program with lookup ports"):
        bpg.ops.air_port_products(3, bpg.ops.memory_trace(5, seed=1), ctl)


# ---------------------------------------------------------------------------------------------- 2. K5


def python_quotient(b, log_n, r, loc, nxt, aux, aux_nxt, ctl, alphas, pos):
    """tests/test_gpu_air_program.py's python_quotient for a program with ports: the program's own constraints, then per
    port l at index n_constraints + 5 l: all rows f f - f; for c = 0, 1 transition z_c - z_c' term_c, last row
    z_c - term_c, with z_c = aux column 2 l + c and term_c = 1 + f (gamma_c + sum_j beta_c^j t_j - 1)."""
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
        base = b.n_constraints + 5 * l
        terms.append((base, ALL_ROWS, (f * f - f) % P))
        for c in range(2):
            v = sum(pow(ctl[2 * c], j, P) * tj for j, tj in enumerate(tup)) % P
            term = (1 + f * (ctl[2 * c + 1] + v - 1)) % P
            z, zn = int(aux[2 * l + c]), int(aux_nxt[2 * l + c])
            terms.append((base + 1 + 2 * c, TRANSITION, (z - zn * term) % P))
            terms.append((base + 2 + 2 * c, LAST_ROW, (z - term) % P))
    assert sorted(i for i, _, _ in terms) == list(range(T))
    return [sum(pow(a, T - 1 - i, P) * sel[kind] * v for i, kind, v in terms) * inv(zh) % P for a in alphas]


def three_units_two_ports():
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
    b.port(b.loc(4) + b.loc(0), [b.loc(5) + 2 * b.loc(6)])
    return b


def degree_nine_quadratic_tuple():
    b = Builder(8, degree=9)
    deep = b.family(1, ALL_ROWS, 9)
    b.unit()
    v = b.loc(1)
    for k in range(8):
        v = v * b.loc(k % 4)
    b.emit(deep, v - b.loc(7))
    b.port(b.loc(0) * b.loc(4), [b.loc(1) * b.loc(2), b.loc(3), b.nxt(5) * b.x])
    return b


@pytest.mark.parametrize("loaded", [0, 1], ids=["spread", "one-pass"])
@pytest.mark.parametrize("log_n", [5, 9])
@pytest.mark.parametrize("make", [three_units_two_ports, degree_nine_quadratic_tuple], ids=["deg3-3units-2ports", "deg9-quadratic-tuple"])
def test_quotient_eval_of_a_program_with_ports_equals_the_fold_over_python_integers(bpg, make, log_n, loaded):
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
    seed = 0xB000 + 16 * log_n + d.degree
    lde, aux = random_lde(8, rows, seed), random_lde(d.n_aux, rows, seed + 1)
    assert d.n_aux == 2 * len(b.ports)
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


# ---------------------------------------------------------------------------------------------- 3. against AIR 3


def exposed_memory_trace(bpg, log_n, seed):
    """ops.memory_trace with the lookup filter g set on a seeded third of the rows"""
    import torch
    t = bpg.ops.memory_trace(log_n, seed=seed)
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    t[pc.MEM_G] = (torch.randint(0, 3, (1 << log_n,), device="cuda", generator=g) == 0).to(torch.int64)
    assert 0 < int(t[pc.MEM_G].sum()) < (1 << log_n)
    return t


def test_memory_port_products_are_the_products_over_python_integers(bpg):
    b = pc.memory_port_program()
    t = exposed_memory_trace(bpg, 6, 0xC006)
    ctl = challenges(0xC100)
    got = to_host(bpg.ops.air_port_products(bpg.ops.air_register(b.assemble()), t, ctl))
    want = pc.port_products(b, to_host(t), ctl)
    assert got.shape == (2, 64) and [[int(v) for v in row] for row in got] == want


@pytest.mark.parametrize("log_n", [6, 13])
def test_memory_port_products_are_the_built_in_product_columns(bpg, log_n):
    """every row, first to last, of both columns: program_port_terms_kernel + the scan against
    aux_suffix_product_kernel<3> (bp_debug_air_aux) on the same trace and challenges"""
    reg = bpg.ops.air_register(pc.memory_port_program().assemble())
    t = exposed_memory_trace(bpg, log_n, 0xC010 + log_n)
    ctl = challenges(0xC110 + log_n)
    want = bpg.ops.debug_air_aux(3, t, ctl)
    got = bpg.ops.air_port_products(reg, t, ctl)
    assert got.shape == want.shape == (2, 1 << log_n) and bool((got == want).all())
    assert int(want[0, 0]) != int(want[1, 0]) and int(want[0, 0]) not in (0, 1)


@pytest.mark.parametrize("loaded", [0, 1], ids=["spread", "one-pass"])
@pytest.mark.parametrize("log_n", [6, 13])
def test_memory_transcription_with_a_port_gives_the_built_in_quotient(bpg, log_n, loaded):
    reg = bpg.ops.air_register(pc.memory_port_program().assemble())
    rows = (1 << log_n) << 1
    trace, aux = random_lde(45, rows, 0xC200 + log_n), random_lde(2, rows, 0xC201 + log_n)
    ctl, alphas = challenges(0xC202 + log_n), challenges(0xC203 + log_n, 2)
    cfg = bpg.ops.stark_cfg(log_n, 45)
    with bpg.ops.tuned(assume_loaded=loaded):
        want = bpg.ops.quotient_eval(cfg, trace, aux, None, ctl, alphas, air_id=3)
        got = bpg.ops.quotient_eval(cfg, trace, aux, None, ctl, alphas, air_id=reg)
    assert got.shape == want.shape == (2, rows)
    assert bool((got == want).all()), "first mismatch at %s" % (got != want).nonzero()[0].tolist()
    assert bool((want != 0).any())


@pytest.mark.parametrize("log_n,nq,pb", [(6, 6, 6), (13, 84, 16)])
def test_memory_transcription_with_a_port_gives_the_built_in_proof(bpg, log_n, nq, pb):
    """every word but header word 14 (the air_id, which is in no transcript): the auxiliary commitment, the openings and
    the quotient of the interpreted port are the built-in lookup's; the proof verifies under its own id only"""
    reg = bpg.ops.air_register(pc.memory_port_program().assemble())
    cfg = cases.cfg_for(3, log_n, num_queries=nq, pow_bits=pb)
    trace = exposed_memory_trace(bpg, log_n, 0xC300 + log_n)
    want = bpg.ops.stark_prove_trace(3, cfg, trace)
    got = bpg.ops.stark_prove_trace(reg, cfg, trace)
    assert got.shape == want.shape and int(got[14]) == reg and int(want[14]) == 3 and int(got[4]) == 2
    assert np.nonzero(got != want)[0].tolist() == [14]
    assert cases.verify(reg, cfg, got) == 0 and cases.verify(3, cfg, want) == 0
    assert cases.verify(3, cfg, got) == -5 and cases.verify(reg, cfg, want) == -5


# ---------------------------------------------------------------------------------------------- 4 .. 6. table sets

def statement(bpg, reg, shapes):
    return [{"air_id": r, "cfg": cfg_of(r, log_n)} for r, log_n in zip(reg, shapes)]


def with_traces(tables, traces):
    return [dict(t, trace=to_dev(tr)) for t, tr in zip(tables, traces)]


def members(container, links):
    """[(offset of the member's four header words, its proof words)] of a "BPGTSET1" container"""
    assert int(container[0]) == int.from_bytes(b"BPGTSET1", "little")
    off = 7 + sum(3 + 2 * len(looking) for looking, _ in links)
    out = []
    for _ in range(int(container[1])):
        n_words = int(container[off + 3])
        out.append((off, container[off + 4:off + 4 + n_words]))
        off += 4 + n_words
    assert off == container.size
    return out


def rejected(bpg, tables, links, container, what=None, code=-5):
    from proof_protocol_decoder_amd._lib import BpgError
    with pytest.raises(BpgError) as e:
        bpg.ops.stark_verify_table_set(tables, links, container)
    assert e.value.code == code and (what is None or what in e.value.message), e.value.message


def test_a_balanced_set_proves_and_verifies_and_every_flipped_bit_is_rejected(bpg):
    from proof_protocol_decoder_amd._lib import BpgError
    reg = bpg.ops.air_register(pc.flag_program().assemble())
    a, b, _, _ = balanced_pair()
    for t in (a, b):
        assert bpg.ops.check_air_trace(reg, to_dev(t)).ok
    tables = statement(bpg, [reg, reg], [5, 7])
    container = bpg.ops.stark_prove_table_set(with_traces(tables, [a, b]), LINK)
    bpg.ops.stark_verify_table_set(tables, LINK, container)
    mem = members(container, LINK)
    assert [int(c) for c in container[:3]] == [int.from_bytes(b"BPGTSET1", "little"), 2, 1]
    for (off, proof), log_n in zip(mem, (5, 7)):
        assert [int(v) for v in container[off:off + 3]] == [reg, log_n, 8]
        assert int(proof[4]) == 2 and int(proof[14]) == reg                 # header word 4: 2 * ports auxiliary columns
    # a member alone is a valid table proof of its own transcript only: not of the lone-table one
    assert cases.verify(reg, tables[0]["cfg"], mem[0][1]) == -5
    # one flipped bit (any of the 64): every word of the prologue and of the members' headers, then seeded positions of the bodies
    at = list(range(7 + 5)) + [off + k for off, _ in mem for k in range(4 + 16)]
    rng = np.random.default_rng(0xD100)
    at += [int(v) for v in rng.integers(0, container.size, size=48)]
    for k in at:
        bad = container.copy()
        bad[k] ^= np.uint64(1 << int(rng.integers(0, 64)))
        with pytest.raises(BpgError):
            bpg.ops.stark_verify_table_set(tables, LINK, bad)
    rejected(bpg, tables, LINK, container[:-1])
    rejected(bpg, tables, LINK, np.concatenate([container, container[:1]]))


def test_two_looking_ports_on_two_tables_into_one_looked_port(bpg):
    reg = bpg.ops.air_register(pc.flag_program().assemble())
    traces, links = pc.two_looking_tables()
    tables = statement(bpg, [reg] * 3, [5, 6, 7])
    container = bpg.ops.stark_prove_table_set(with_traces(tables, traces), links)
    bpg.ops.stark_verify_table_set(tables, links, container)
    assert [int(p[4]) for _, p in members(container, links)] == [2, 2, 2]
    # the two looking ports exchanged name the same multiset, but another statement: the transcript differs
    rejected(bpg, tables, [([(1, 0), (0, 0)], (2, 0))], container)


@pytest.mark.parametrize("case", ["cell", "stranger", "unflagged"])
def test_a_set_that_does_not_balance_is_refused_by_the_prover_and_the_verifier(bpg, case):
    from proof_protocol_decoder_amd._lib import BpgError
    reg = bpg.ops.air_register(pc.flag_program().assemble())
    a, b, a_rows, b_rows = balanced_pair()
    if case == "cell":          # one tuple cell changed on a flagged row of A
        a[2, a_rows[4]] = (int(a[2, a_rows[4]]) + 1) % P
    elif case == "stranger":    # the tuple sent twice is exposed once, next to a stranger
        twice = [r for r in b_rows if [int(v) for v in b[1:1 + WIDTH, r]] == [int(v) for v in a[1:1 + WIDTH, a_rows[3]]]]
        assert len(twice) == 2
        b[1, twice[1]] = (int(b[1, twice[1]]) + 12345) % P
    else:                       # a flagged row of B unflagged
        b[0, b_rows[7]] = 0
    tables = statement(bpg, [reg, reg], [5, 7])
    for t, tr in zip(tables, (a, b)):   # each table is still valid alone
        assert bpg.ops.check_air_trace(reg, to_dev(tr)).ok
        assert cases.verify(reg, t["cfg"], bpg.ops.stark_prove_trace(reg, t["cfg"], to_dev(tr))) == 0
    with pytest.raises(BpgError) as e:
        bpg.ops.stark_prove_table_set(with_traces(tables, [a, b]), LINK)
    assert e.value.code == -5 and "link 0 does not hold" in e.value.message and "port 0 of table 0" in e.value.message \
        and "port 0 of table 1" in e.value.message, e.value.message
    container = bpg.ops.stark_prove_table_set(with_traces(tables, [a, b]), LINK, skip_link_check=True)
    rejected(bpg, tables, LINK, container, "link 0 does not hold")
    assert b"link 0" in bpg.lib().bp_last_error()


def test_a_filter_that_is_no_bit_is_rejected_at_zeta(bpg):
    """the flag column of this table has no constraint of its own: the port's f f - f is the only one that sees the 2"""
    b = Builder(8)
    count = b.family(1, TRANSITION, 1)
    b.unit()
    b.emit(count, b.nxt(4) - b.loc(4) - 1)
    b.port(b.loc(0), [b.loc(1 + j) for j in range(WIDTH)])
    loose = bpg.ops.air_register(b.assemble())
    a, bb, a_rows, _ = balanced_pair()
    cfg = cfg_of(loose, 5)
    assert cases.verify(loose, cfg, bpg.ops.stark_prove_trace(loose, cfg, to_dev(a))) == 0
    a[0, a_rows[2]] = 2
    assert bpg.ops.check_air_trace(loose, to_dev(a)).ok                      # the checker drops the ports
    assert cases.verify(loose, cfg, bpg.ops.stark_prove_trace(loose, cfg, to_dev(a))) == -5
    assert b"constraint check at zeta" in bpg.lib().bp_last_error()
    reg = bpg.ops.air_register(pc.flag_program().assemble())
    tables = [{"air_id": loose, "cfg": cfg}, {"air_id": reg, "cfg": cfg_of(reg, 7)}]
    container = bpg.ops.stark_prove_table_set(with_traces(tables, [a, bb]), LINK, skip_link_check=True)
    rejected(bpg, tables, LINK, container, "table 0: constraint check at zeta")


def test_the_statement_is_the_verifiers(bpg):
    reg = bpg.ops.air_register(pc.flag_program().assemble())
    # two same-shaped ports on each side: A sends on ports 0 and 1 (port 1's tuple is port 0's + 1), B exposes both
    two = bpg.ops.air_register(pc.flag_program(ports=2).assemble())
    rng = np.random.default_rng(0xD300)
    sent = [[int(v) for v in field(rng, WIDTH)] for _ in range(7)]
    a, b = flagged(5, rows_of(5, rng, 7), sent, rng), flagged(5, rows_of(5, rng, 7), [sent[k] for k in rng.permutation(7)], rng)
    tables = statement(bpg, [two, two], [5, 5])
    links = [([(0, 0)], (1, 0)), ([(0, 1)], (1, 1))]
    container = bpg.ops.stark_prove_table_set(with_traces(tables, [a, b]), links)
    bpg.ops.stark_verify_table_set(tables, links, container)
    # the link's two ends exchanged between two same-shaped ports: balanced too, but not what was proven
    rejected(bpg, tables, [([(1, 0)], (0, 0)), ([(0, 1)], (1, 1))], container)
    rejected(bpg, tables, [([(0, 0)], (1, 1)), ([(0, 1)], (1, 0))], container)
    # another registered program of the same shape in A's place: the digest is in the transcript
    other = pc.flag_program(ports=2)
    other.units[0].append((0, other.const(0) * other.loc(1)))                # one more (vanishing) emit: other bytes
    other_id = bpg.ops.air_register(other.assemble())
    assert other_id != two and bpg.ops.air_program_digest(other_id) != bpg.ops.air_program_digest(two)
    swapped = [dict(tables[0], air_id=other_id), tables[1]]
    rejected(bpg, swapped, links, container, "table 0 is proven as")
    relabelled = container.copy()
    off = members(container, links)[0][0]
    relabelled[off] = other_id
    relabelled[off + 4 + 14] = other_id                                      # ... and header word 14 of the member
    rejected(bpg, swapped, links, relabelled, "lookup challenges do not follow")
    # log_n changed
    rejected(bpg, [dict(tables[0], cfg=cfg_of(two, 6)), tables[1]], links, container, "table 0 is proven as")
    a1, b1, _, _ = balanced_pair()
    t57 = statement(bpg, [reg, reg], [5, 7])
    c57 = bpg.ops.stark_prove_table_set(with_traces(t57, [a1, b1]), LINK)
    rejected(bpg, statement(bpg, [reg, reg], [5, 6]), LINK, c57, "table 1 is proven as")


# ---------------------------------------------------------------------------------------------- 7. into a built-in


def test_a_run_time_table_looks_words_up_in_the_built_in_memory_table(bpg):
    from proof_protocol_decoder_amd._lib import BpgError
    tables, (r, mem) = pc.memory_readers(bpg)
    reader = tables[0]["air_id"]
    container = bpg.ops.stark_prove_table_set([dict(tables[0], trace=to_dev(r)), dict(tables[1], trace=mem)], LINK)
    bpg.ops.stark_verify_table_set(tables, LINK, container)
    assert [int(p[14]) for _, p in members(container, LINK)] == [reader, 3]
    # a value the log does not hold
    row = next(i for i in range(32) if r[0, i] == 1)
    r[1 + 5, row] ^= np.uint64(1)
    with pytest.raises(BpgError) as e:
        bpg.ops.stark_prove_table_set([dict(tables[0], trace=to_dev(r)), dict(tables[1], trace=mem)], LINK)
    assert e.value.code == -5 and "link 0 does not hold" in e.value.message and "port 0 of table 1" in e.value.message
