"""Seeded random run-time AIRs for tests/test_air_program.py and tests/test_gpu_air_program.py, built only on the Python
builder (proof_protocol_decoder_amd/air_program.py): Builder.evaluate() over Python integers is the reference of
everything these programs are used for.

A program is satisfiable by construction.  Columns [0, n_free) are free; constraint i is  E_i - loc(n_free + i)  with E_i a
random expression over the free columns only (loc, nxt, cst, pub, x, immediates, + - *) whose degree is exactly its
family's bound, so a witness is: free columns at random, slack column n_free + i = E_i row by row -- and, on the rows
where constraint i's kind is switched off, a random word that is NOT E_i, so that a selector that masked nothing would
be seen.  Every property a case is in the list for (degree, registers, units, opcodes, kinds) is asserted here: a change
to the builder cannot silently move a case off its path."""
import functools

import numpy as np

from proof_protocol_decoder_amd.air_program import (ALL_ROWS, FIRST_ROW, LAST_ROW, MAX_REGS, OP_EMIT, OP_IMM, P, TRANSITION,
                                                    Builder)
from util import rand_field

EDGE_IMMEDIATES = (0, 1, 2, P - 1, 1 << 32, (1 << 32) - 1)
KINDS = (ALL_ROWS, TRANSITION, FIRST_ROW, LAST_ROW)


def boundary_degree_cap(degree):
    """the degree a first-row or last-row family may have in a program of `degree` (include/bpg.h, "Run-time AIRs"): the
    selector is a Lagrange polynomial of degree n - 1, and (d + 1)(n - 1) - n < 2^rate_bits n needs d <= 2^rate_bits"""
    return 2 if degree <= 3 else 8


class _UncheckedBuilder(Builder):
    """writes the words of a program that bp_air_register is expected to refuse: the cases that probe the rule above"""

    def _check_boundary(self, kind, degree, program_degree):
        pass


class _Gen:
    """random expressions over the free columns of one builder, of an exact formal degree"""

    def __init__(self, b, rng, n_free):
        self.b, self.rng, self.n_free = b, rng, n_free
        # leaves every program must contain, handed out before random ones
        self.must1 = [("cst", k) for k in range(b.n_const)] + [("x", 0), ("nxt", 0), ("nxt", n_free - 1)]
        self.must0 = [("pub", j) for j in range(b.n_public)] + [("imm", v) for v in EDGE_IMMEDIATES]

    def _leaf(self, what, k):
        b = self.b
        return {"cst": b.cst, "nxt": b.nxt, "loc": b.loc, "pub": b.pub, "imm": b.const}[what](k) if what != "x" else b.x

    def leaf1(self, allow_nxt):
        for i, (what, k) in enumerate(self.must1):
            if allow_nxt or what != "nxt":
                del self.must1[i]
                return self._leaf(what, k)
        r = int(self.rng.integers(0, 10))
        col = int(self.rng.integers(0, self.n_free))
        if r < 5 or (r < 8 and not allow_nxt):
            return self.b.loc(col)
        if r < 8:
            return self.b.nxt(col)
        if r == 8 and self.b.n_const:
            return self.b.cst(int(self.rng.integers(0, self.b.n_const)))
        return self.b.x

    def leaf0(self):
        if self.must0:
            return self._leaf(*self.must0.pop(0))
        if self.b.n_public and self.rng.integers(0, 3) == 0:
            return self.b.pub(int(self.rng.integers(0, self.b.n_public)))
        return self.b.const(int(rand_field(self.rng, (1,), edge=False)[0]))

    def with_scalar(self, e):
        """e combined with a degree-0 leaf in a way the builder does not fold away (0 + e, e * 1, ...)"""
        s = self.leaf0()
        ops = ["add", "sub", "mul"]
        if s.op == OP_IMM and s.a == 0:
            ops = ["sub", "mul"]          # 0 - e, 0 * e
        elif s.op == OP_IMM and s.a == 1:
            ops = ["add", "sub"]          # 1 + e, 1 - e
        op = ops[int(self.rng.integers(0, len(ops)))]
        return s + e if op == "add" else s - e if op == "sub" else s * e

    def expr(self, d, allow_nxt=True):
        """a random expression of formal degree exactly d >= 1"""
        if d == 1:
            e = self.leaf1(allow_nxt)
            r = int(self.rng.integers(0, 4))
            if r == 0:
                e = e + self.leaf1(allow_nxt)
            elif r == 1:
                e = e - self.leaf1(allow_nxt)
        else:
            a = int(self.rng.integers(1, d))
            e = self.expr(a, allow_nxt) * self.expr(d - a, allow_nxt)
            if self.rng.integers(0, 3) == 0:
                e = e + self.expr(int(self.rng.integers(1, d + 1)), allow_nxt)
        if self.must0 or self.rng.integers(0, 3) == 0:
            e = self.with_scalar(e)
        assert e.degree == d, (e.degree, d)
        return e


def _build(seed, degree, n_units, live, n_const, n_public, n_families, per_family, n_free, boundary_degree):
    rng = np.random.default_rng(seed)
    assert n_families >= 4 and per_family >= 1 and n_free >= 8
    kinds = list(KINDS) + [int(k) for k in rng.integers(0, 4, size=n_families - 4)]
    rng.shuffle(kinds)
    cap = boundary_degree_cap(degree)
    degs = []
    for k in kinds:
        d = int(rng.integers(1, degree + 1))
        if k in (FIRST_ROW, LAST_ROW):
            d = min(d, cap) if boundary_degree is None else boundary_degree
        degs.append(d)
    if boundary_degree is None:
        # a family of the program's degree, and boundary families AT their cap: the edge of what the rule allows
        degs[next(i for i, k in enumerate(kinds) if k in (ALL_ROWS, TRANSITION))] = degree
        degs[kinds.index(FIRST_ROW)] = min(degree, cap)
        degs[kinds.index(LAST_ROW)] = min(degree, cap)
    counts = [int(c) for c in rng.integers(max(1, per_family - 2), per_family + 3, size=n_families)]
    n_constraints = sum(counts)
    assert n_constraints >= 2 * n_units, "every unit gets at least two emits"
    make_builder = Builder if boundary_degree is None else _UncheckedBuilder
    b = make_builder(n_free + n_constraints, n_const=n_const, n_public=n_public, degree=degree)
    for c, k, d in zip(counts, kinds, degs):
        b.family(c, k, d)
    g = _Gen(b, rng, n_free)
    fam_of = [f for f in b.families for _ in range(f[1])]
    order = [int(i) for i in rng.permutation(n_constraints)]
    units = [order[u::n_units] for u in range(n_units)]          # dealt in shuffled order
    # register pressure: `live` distinct non-leaf values that the widest unit's first emit defines and its last reads
    wide = max(range(n_units), key=lambda u: len(units[u]))
    held = [b.loc(int(rng.integers(0, n_free))) + (k + 3) * b.loc(int(rng.integers(0, n_free))) for k in range(live)]
    # indices whose expression is split into two summands emitted from two different units (one unit: emitted twice)
    split = {units[u][0]: (u + 1) % n_units for u in range(min(n_units, 3))}          # index -> the second unit
    extra = {u: [] for u in range(n_units)}
    emits = {}
    for u in range(n_units):
        for pos, i in enumerate(units[u]):
            _, _, kind, d = fam_of[i]
            allow_nxt = kind != LAST_ROW
            e = g.expr(d, allow_nxt)
            if u == wide and held and pos == 0:
                for v in held:
                    e = e + v
            if u == wide and held and pos == len(units[u]) - 1:
                for k, v in enumerate(held):
                    e = e - (k + 2) * v
            assert e.degree == d
            if i in split:
                extra[split[i]].append((i, g.expr(int(rng.integers(1, d + 1)), allow_nxt)))
            emits[(u, i)] = e - b.loc(n_free + i)
    for u in range(n_units):
        b.unit()
        first = units[u][0]
        b.emit(first, emits[(u, first)])
        for i, e in extra[u]:
            b.emit(i, e)
        for i in units[u][1:]:
            b.emit(i, emits[(u, i)])
    assert not g.must1 and not g.must0, "a mandatory leaf was not placed"
    return b, n_free, n_constraints, sorted(split)


def make(seed, degree, n_units, live=0, n_const=1, n_public=1, n_families=6, per_family=3, n_free=12, boundary_degree=None):
    """(builder, n_free, n_constraints).  `live` is lowered until assemble() stays within the library's 64 registers.
    boundary_degree: None = first-row and last-row families keep to boundary_degree_cap(degree); a number = they all get
    exactly that degree (the cases that probe the rule)."""
    while True:
        b, n_free, n_constraints, split = _build(seed, degree, n_units, live, n_const, n_public, n_families, per_family, n_free,
                                                 boundary_degree)
        try:
            b.assemble()
            break
        except ValueError as e:
            if "registers" not in str(e) or live == 0:
                raise
            live -= 1
    b.split_indices, b.live = split, live
    return b, n_free, n_constraints


# ---------------------------------------------------------------------------------------------- what a program is made of


def header(words):
    names = ("n_cols", "n_const", "n_public", "degree", "n_constraints", "n_families", "n_regs", "n_units", "n_code")
    return dict(zip(names, (int(w) for w in words[1:10])))


def instructions(words):
    """[(unit, op, dst, a, b, constant or None)] of a program's code"""
    h = header(words)
    off0 = 10 + 4 * h["n_families"]
    code0 = off0 + h["n_units"] + 1
    out = []
    for u in range(h["n_units"]):
        pc, end = code0 + int(words[off0 + u]), code0 + int(words[off0 + u + 1])
        while pc < end:
            c = int(words[pc])
            op = c & 0xFF
            out.append((u, op, (c >> 8) & 0xFF, (c >> 16) & 0xFFFFFF, c >> 40, int(words[pc + 1]) if op == OP_IMM else None))
            pc += 2 if op == OP_IMM else 1
    return out


def check_program(b, words, degree, n_units, boundary_cap=True):
    """the properties every generated program has: its degree is reached, all ten operations, all four kinds, every
    input, the edge immediates, an index fed from two units, boundary families within (and at) their cap"""
    h = header(words)
    ins = instructions(words)
    assert h["degree"] == degree == max(f[3] for f in b.families) and h["n_units"] == n_units
    assert {i[1] for i in ins} == set(range(10)), "not every operation is used"
    assert {i[2] for i in ins if i[1] == OP_EMIT} == set(KINDS), "not every kind is emitted"
    assert {f[2] for f in b.families} == set(KINDS)
    assert {i[3] for i in ins if i[1] == 2} == set(range(b.n_const)), "not every constant column is read"
    assert {i[3] for i in ins if i[1] == 3} == set(range(b.n_public)), "not every public input is read"
    assert set(EDGE_IMMEDIATES) <= {i[5] for i in ins if i[1] == OP_IMM}
    units_of = {}
    for i in ins:
        if i[1] == OP_EMIT:
            units_of.setdefault(i[3], []).append(i[0])
    assert sorted(units_of) == list(range(h["n_constraints"]))
    several = sorted(i for i, us in units_of.items() if len(us) > 1 and (len(set(us)) > 1 or n_units == 1))
    assert several and several == b.split_indices, "no index is emitted from two units"
    if boundary_cap:
        cap = boundary_degree_cap(degree)
        bd = [f[3] for f in b.families if f[2] in (FIRST_ROW, LAST_ROW)]
        assert max(bd) == min(cap, degree) and all(d <= cap for d in bd)
    assert h["n_regs"] <= MAX_REGS


class Case:
    """one program of the fixed list: the builder, its words and the properties it is in the list for (asserted)"""

    def __init__(self, name, want_regs=None, tall=False, boundary_cap=True, **kw):
        self.name, self.tall, self.kw = name, tall, kw
        self.b, self.n_free, self.n_constraints = make(**kw)
        self.words = self.b.assemble()
        self.n_regs = header(self.words)["n_regs"]
        self.degree, self.n_units = kw["degree"], kw["n_units"]
        self.deg_pow, self.rate_bits = (3, 3) if self.degree > 3 else (1, 1)
        check_program(self.b, self.words, self.degree, self.n_units, boundary_cap)
        if want_regs:
            assert want_regs[0] <= self.n_regs <= want_regs[1], "%s: %d registers, wanted %s" % (name, self.n_regs, want_regs)

    def __repr__(self):
        return "Case(%s: degree %d, %d units, %d registers, %d constraints, %d nodes)" % (
            self.name, self.degree, self.n_units, self.n_regs, self.n_constraints, len(self.b._order))


# name -> (keyword arguments of make, registers asserted, runs at 2^15 as well)
_SPECS = {
    "deg1-u1": (dict(seed=101, degree=1, n_units=1), None, False),
    "deg2-u3": (dict(seed=102, degree=2, n_units=3), None, False),
    "deg3-u5": (dict(seed=103, degree=3, n_units=5, n_families=7), None, True),
    "deg4-u12": (dict(seed=104, degree=4, n_units=12, n_families=8, per_family=4), None, False),
    "deg5-u1": (dict(seed=105, degree=5, n_units=1), None, False),
    "deg7-u3": (dict(seed=107, degree=7, n_units=3), None, True),
    "deg9-u5": (dict(seed=109, degree=9, n_units=5, n_families=7), None, False),
    "regs-large-a": (dict(seed=201, degree=3, n_units=2, live=60, per_family=4), (57, 64), False),
    "regs-large-b": (dict(seed=202, degree=7, n_units=3, live=60, per_family=4), (57, 64), False),
    "regs-mid": (dict(seed=203, degree=2, n_units=2, live=30), (33, 40), False),
    "units40": (dict(seed=204, degree=2, n_units=40, n_families=24, per_family=88, n_free=16), None, False),
    "inputs": (dict(seed=205, degree=4, n_units=4, n_const=4, n_public=4, n_families=8), None, False),
}
CASES = sorted(_SPECS)
# The boundary-degree probes: a first-row and a last-row family of the program's own degree, above the cap.
_PROBES = {
    "first-row-deg3": dict(seed=301, degree=3, n_units=2, boundary_degree=3),
    "first-row-deg9": dict(seed=302, degree=9, n_units=2, boundary_degree=9),
}
PROBES = sorted(_PROBES)


@functools.lru_cache(maxsize=None)
def case(name):
    if name in _PROBES:
        c = Case(name, boundary_cap=False, **_PROBES[name])
        assert all(f[3] == c.degree for f in c.b.families if f[2] in (FIRST_ROW, LAST_ROW))
        return c
    kw, regs, tall = _SPECS[name]
    c = Case(name, want_regs=regs, tall=tall, **kw)
    if name == "units40":
        assert c.n_units == 40 and c.n_constraints >= 2000 and c.degree <= 2
    if name == "inputs":
        assert (c.b.n_const, c.b.n_public) == (4, 4)
    if name == "regs-large-a":
        assert c.degree <= 3
    if name == "regs-large-b":
        assert c.degree >= 4
    return c


# ---------------------------------------------------------------------------------------------- witnesses


def domain(log_n):
    """[w_n^i] of the trace domain"""
    w, x, out = pow(7, (P - 1) >> log_n, P), 1, []
    for _ in range(1 << log_n):
        out.append(x)
        x = x * w % P
    return out


def evaluate_columns(b, trace, consts, pub, xs, rows=None):
    """Builder.evaluate()'s walk for many rows at once (`rows`: a range; default all): numpy OBJECT arrays, so every
    operation is still Python's integer arithmetic mod p (no 64-bit arithmetic anywhere); witness() checks rows of it
    against evaluate() itself.  Returns [n_constraints] arrays of len(rows) Python integers."""
    n = trace.shape[1]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    m = len(rows)
    obj = lambda a: np.array([int(v) for v in a], dtype=object)
    val = [None] * len(b._order)
    for e in b._order:
        if e.op == 0:
            v = obj(trace[e.a][rows])
        elif e.op == 1:
            v = obj(trace[e.a][(rows + 1) % n])
        elif e.op == 2:
            v = obj(consts[e.a][rows])
        elif e.op == 3:
            v = np.array([int(pub[e.a])] * m, dtype=object)
        elif e.op == 4:
            v = np.array([xs[r] for r in rows], dtype=object)
        elif e.op == 5:
            v = np.array([e.a] * m, dtype=object)
        elif e.op == 6:
            v = (val[e.a.n] + val[e.c.n]) % P
        elif e.op == 7:
            v = (val[e.a.n] - val[e.c.n]) % P
        else:
            v = (val[e.a.n] * val[e.c.n]) % P
        val[e.n] = v
    out = [np.array([0] * m, dtype=object) for _ in range(b.n_constraints)]
    for u in b.units:
        for index, e in u:
            out[index] = (out[index] + val[e.n]) % P
    return out


def active(kind, i, n):
    return kind == ALL_ROWS or (kind == TRANSITION and i != n - 1) or (kind == FIRST_ROW and i == 0) or (kind == LAST_ROW and i == n - 1)


@functools.lru_cache(maxsize=None)
def witness(name, log_n):
    """(trace [n_cols, n], constants [n_const, n] or None, four public inputs or None) of case `name`, uint64: a valid
    witness whose slack cells are wrong wherever their constraint's kind is switched off"""
    c = case(name)
    b, n = c.b, 1 << log_n
    rng = np.random.default_rng([c.kw["seed"], log_n])
    trace = np.zeros((b.n_cols, n), dtype=np.uint64)
    trace[:c.n_free] = rand_field(rng, (c.n_free, n))
    consts = rand_field(rng, (b.n_const, n)) if b.n_const else None
    pub = ([int(v) for v in rand_field(rng, (b.n_public,), edge=False)] + [0] * 4)[:4] if b.n_public else None
    xs = domain(log_n)
    step = max(1, min(n, (1 << 21) // len(b._order)))              # (bounds the walk's memory: 2^21 values at a time)
    values = [np.zeros(n, dtype=np.uint64) for _ in range(b.n_constraints)]
    for r0 in range(0, n, step):                                  # the slack columns are zero: constraint i is E_i
        for i, v in enumerate(evaluate_columns(b, trace, consts, pub, xs, range(r0, min(n, r0 + step)))):
            values[i][r0:r0 + step] = [int(w) for w in v]
    garbage = rand_field(rng, (b.n_constraints, n), edge=False)
    for first, count, kind, _ in b.families:
        for i in range(first, first + count):
            col = values[i]
            if kind != ALL_ROWS:
                off = np.array([not active(kind, r, n) for r in range(n)])
                wrong = np.where(garbage[i] == 0, np.uint64(5), garbage[i])          # non-zero, and not E_i
                wrong = np.where(wrong == col, wrong ^ np.uint64(1), wrong)
                col = np.where(off, wrong, col)
            trace[c.n_free + i] = col
    # rows of the vectorised walk against evaluate() itself: the first, the last (its next row is row 0) and random ones
    for r in sorted({0, 1, n - 2, n - 1} | {int(v) for v in rng.integers(0, n, size=4)}):
        vals = b.evaluate(trace[:, r], trace[:, (r + 1) % n], consts[:, r] if consts is not None else (), pub or (), xs[r])
        for first, count, kind, _ in b.families:
            for i in range(first, first + count):
                assert (vals[i] == 0) == active(kind, r, n), (name, log_n, r, i, kind)
    for a in (trace, consts):
        if a is not None:
            a.setflags(write=False)
    return trace, consts, pub


def violations(b, trace, consts, pub, rows=None):
    """(row, constraint, family, kind, value) of every non-zero constraint that the trace domain's selectors leave on, on
    `rows` (default: all), from Builder.evaluate() over Python integers"""
    n = trace.shape[1]
    xs = domain(n.bit_length() - 1)
    out = []
    for i in (range(n) if rows is None else rows):
        vals = b.evaluate(trace[:, i], trace[:, (i + 1) % n], consts[:, i] if consts is not None else (), pub or (), xs[i])
        for fi, (first, count, kind, _) in enumerate(b.families):
            if active(kind, i, n):
                out += [(i, first + j, fi, kind, vals[first + j]) for j in range(count) if vals[first + j]]
    return out


def active_cell(c, kind, n, rng):
    """(row, column) of a slack cell of a constraint of `kind` on a row where that kind is switched on"""
    fams = [f for f in c.b.families if f[2] == kind]
    first, count, _, _ = fams[int(rng.integers(0, len(fams)))]
    i = first + int(rng.integers(0, count))
    row = {ALL_ROWS: int(rng.integers(0, n)), TRANSITION: int(rng.integers(0, n - 1)), FIRST_ROW: 0, LAST_ROW: n - 1}[kind]
    return row, c.n_free + i


def honest_quotient_degree(name, log_n=5, alpha=0x1234567890ABCDEF):
    """The degree of the quotient polynomial of case `name`'s constructed witness, over Python integers: the columns
    interpolated (a plain O(n^2) DFT), the constraints folded with one challenge and divided by Z_H on a coset TWICE
    the size the prover uses, the quotient interpolated from those values.  A proof holds n << rate_bits of its
    coefficients."""
    c = case(name)
    trace, consts, pub = witness(name, log_n)
    n, b = 1 << log_n, c.b
    big = n << (c.rate_bits + 1)
    inv = lambda v: pow(v % P, P - 2, P)
    g, wb = pow(7, (P - 1) >> log_n, P), pow(7, (P - 1) // big, P)

    def coefficients(values, root, size, shift=1):
        values = [int(v) for v in values]
        return [sum(values[i] * pow(root, -i * k % size, P) for i in range(size)) * inv(size) * pow(inv(shift), k, P) % P
                for k in range(size)]

    def at(cf, x):
        acc = 0
        for k in reversed(cf):
            acc = (acc * x + k) % P
        return acc

    tc, cc = [coefficients(col, g, n) for col in trace], [coefficients(col, g, n) for col in consts]
    q = []
    for i in range(big):
        x = 7 * pow(wb, i, P) % P
        vals = b.evaluate([at(cf, x) for cf in tc], [at(cf, g * x % P) for cf in tc], [at(cf, x) for cf in cc], pub, x)
        zh = (pow(x, n, P) - 1) % P
        sel = [1, (x - inv(g)) % P, zh * inv(n * (x - 1)) % P, zh * inv(n * (g * x - 1)) % P]
        fold = sum(pow(alpha, b.n_constraints - 1 - k, P) * sel[f[2]] * vals[k] for f in b.families for k in range(f[0], f[0] + f[1]))
        q.append(fold * inv(zh) % P)
    cf = coefficients(q, wb, big, shift=7)
    return max(k for k in range(big) if cf[k])
