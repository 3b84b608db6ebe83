"""A builder for run-time AIRs: constraint programs for bp_air_register (include/bpg.h, csrc/air_program.hpp).

    b = Builder(n_cols=8, n_const=1, n_public=2)
    first = b.family(1, kind=FIRST_ROW, degree=1)       # the constraint list, family by family, in index order
    step = b.family(2, kind=TRANSITION, degree=1)
    b.unit()                                            # units: what the kernel spreads over grid.y
    b.emit(first, b.loc(0) - b.pub(0))
    b.emit(step, b.nxt(0) - b.loc(1))
    b.emit(step + 1, b.nxt(1) - (b.loc(0) + b.loc(1)))
    words = b.assemble()                                # numpy uint64: the program bytes
    values = b.evaluate(row, next_row)                  # the same constraints over Python integers

A lookup PORT makes the table a side of a cross-table lookup (AIRS.md section 3, "Run-time lookups"):

    p = b.port(b.loc(7), [b.loc(0), b.loc(1) + b.nxt(1)])   # filter, tuple; returns the port's index
    words = b.assemble()                                # a builder with a port assembles "BPGAIRP2"
    (f, t), = b.evaluate_ports(row, next_row)           # the filter and the tuple over Python integers

The program only states the filter and the tuple; the two running products of the port and their five constraints are
the library's (include/bpg.h).  A builder without a port assembles the "BPGAIRP1" bytes it always did.

A LOG port's running columns are sums of fractions f / (gamma + v) instead of products, so its filter may be a
multiplicity -- which is what a range check needs (AIRS.md section 3, "Log links and range checks"):

    for k in range(8):
        b.log_port(b.loc(8), [b.loc(k)])                    # the rows where loc(8) is 1 send limb k; the library adds f f - f
    b.log_port(b.loc(9), [b.cst(0)], multiplicity=True)     # constant column 0 .. 2^k - 1, loc(9) = how often each is asked for
    words = b.assemble()                                    # a builder with a log port assembles "BPGAIRP3"
    cols = b.port_running_columns(trace, ctl, consts)       # every port's two running columns over Python integers

Expressions are built from loc(c), nxt(c), cst(c), pub(j), x and integers with + - *; equal subexpressions are one node
(hash-consing), so a value used twice in a unit is computed once.  assemble() schedules every unit's emits in order,
allocates registers by last use (a leaf -- a load or a constant -- is re-issued for each emit instead of being kept, which
keeps n_regs, and with it the kernel's LDS footprint, small) and writes the words.  evaluate() walks the same expression
graph over Python integers mod p: it shares nothing with the library's interpreter, which is what makes it a check of it.
"""
import numpy as np

P = 2 ** 64 - 2 ** 32 + 1
MAGIC = int.from_bytes(b"BPGAIRP1", "little")
MAGIC2 = int.from_bytes(b"BPGAIRP2", "little")
MAGIC3 = int.from_bytes(b"BPGAIRP3", "little")
PORT_PRODUCT, PORT_LOG_BIT, PORT_LOG_MULT = 0, 1, 2   # a port's kind: "BPGAIRP3" carries it in the port word, << 32
OP_PORT = 10
MAX_PORTS, MAX_TUPLE, MAX_FAMILIES_WITH_PORTS = 8, 128, 21
ALL_ROWS, TRANSITION, FIRST_ROW, LAST_ROW = 0, 1, 2, 3
OP_LOC, OP_NXT, OP_CST, OP_PUB, OP_X, OP_IMM, OP_ADD, OP_SUB, OP_MUL, OP_EMIT = range(10)
MAX_REGS = 64
_LEAVES = (OP_LOC, OP_NXT, OP_CST, OP_PUB, OP_X, OP_IMM)


def boundary_degree(degree):
    """The degree a first-row or last-row family may have in a program of `degree`.  Those rows' selectors are Lagrange
    polynomials of degree n - 1, so a family of degree d leaves a quotient of degree (d + 1)(n - 1) - n, and the
    2^rate_bits n quotient coefficients (rate_bits 1 up to degree 3, else 3) hold that only for d <= 2^rate_bits."""
    return 2 if degree <= 3 else 8


class Expr:
    """One node of a builder's expression graph (make them with the builder's loc / nxt / cst / pub / x / const)."""
    __slots__ = ("b", "op", "a", "c", "degree", "n")

    def __init__(self, b, op, a, c, degree, n):
        self.b, self.op, self.a, self.c, self.degree, self.n = b, op, a, c, degree, n

    def __add__(self, o):
        return self.b._bin(OP_ADD, self, o)

    def __radd__(self, o):
        return self.b._bin(OP_ADD, o, self)

    def __sub__(self, o):
        return self.b._bin(OP_SUB, self, o)

    def __rsub__(self, o):
        return self.b._bin(OP_SUB, o, self)

    def __mul__(self, o):
        return self.b._bin(OP_MUL, self, o)

    def __rmul__(self, o):
        return self.b._bin(OP_MUL, o, self)

    def __neg__(self):
        return self.b._bin(OP_SUB, 0, self)


class Builder:
    def __init__(self, n_cols, n_const=0, n_public=0, degree=None):
        self.n_cols, self.n_const, self.n_public, self.degree = n_cols, n_const, n_public, degree
        self.families = []   # (first_index, count, kind, degree)
        self.units = []      # lists of (index, Expr)
        self.ports = []      # (filter Expr, [tuple Exprs])
        self.port_kinds = []  # per port PORT_PRODUCT / PORT_LOG_BIT / PORT_LOG_MULT
        self._nodes = {}     # key -> Expr
        self._order = []     # every node, operands before users

    # ---- expressions
    def _node(self, op, a, c, degree):
        key = (op, a.n if isinstance(a, Expr) else a, c.n if isinstance(c, Expr) else c)
        e = self._nodes.get(key)
        if e is None:
            e = self._nodes[key] = Expr(self, op, a, c, degree, len(self._order))
            self._order.append(e)
        return e

    def loc(self, c):
        assert 0 <= c < self.n_cols, "column %d of %d" % (c, self.n_cols)
        return self._node(OP_LOC, c, None, 1)

    def nxt(self, c):
        assert 0 <= c < self.n_cols, "column %d of %d" % (c, self.n_cols)
        return self._node(OP_NXT, c, None, 1)

    def cst(self, c):
        assert 0 <= c < self.n_const, "constant column %d of %d" % (c, self.n_const)
        return self._node(OP_CST, c, None, 1)

    def pub(self, j):
        assert 0 <= j < self.n_public, "public input %d of %d" % (j, self.n_public)
        return self._node(OP_PUB, j, None, 0)

    @property
    def x(self):
        return self._node(OP_X, None, None, 1)

    def const(self, v):
        return self._node(OP_IMM, int(v) % P, None, 0)

    def _bin(self, op, a, c):
        a = a if isinstance(a, Expr) else self.const(a)
        c = c if isinstance(c, Expr) else self.const(c)
        assert a.b is self and c.b is self, "expressions of another builder"
        if a.op == OP_IMM and c.op == OP_IMM:
            return self.const({OP_ADD: a.a + c.a, OP_SUB: a.a - c.a, OP_MUL: a.a * c.a}[op])
        if op == OP_ADD and a.op == OP_IMM and a.a == 0:
            return c
        if op in (OP_ADD, OP_SUB) and c.op == OP_IMM and c.a == 0:
            return a
        if op == OP_MUL and a.op == OP_IMM and a.a == 1:
            return c
        if op == OP_MUL and c.op == OP_IMM and c.a == 1:
            return a
        return self._node(op, a, c, a.degree + c.degree if op == OP_MUL else max(a.degree, c.degree))

    # ---- the constraint list and the units
    @property
    def n_constraints(self):
        return sum(f[1] for f in self.families)

    def family(self, count, kind=ALL_ROWS, degree=2):
        """The next `count` constraint indices, of one kind and degree bound; returns the first of them."""
        if self.degree is not None:
            self._check_boundary(kind, degree, self.degree)
        first = self.n_constraints
        self.families.append((first, count, kind, degree))
        return first

    def _check_boundary(self, kind, degree, program_degree):
        """bp_air_register's rule for first-row and last-row families (boundary_degree)"""
        if kind in (FIRST_ROW, LAST_ROW) and degree > boundary_degree(program_degree):
            raise ValueError("a first-row or last-row family of degree %d: a program of degree %d takes them up to degree %d"
                             % (degree, program_degree, boundary_degree(program_degree)))

    def unit(self):
        """Starts the next unit; the emits that follow belong to it.  Returns its number."""
        self.units.append([])
        return len(self.units) - 1

    def _family_of(self, index):
        for f in self.families:
            if f[0] <= index < f[0] + f[1]:
                return f
        raise ValueError("constraint %d is in no family" % index)

    def emit(self, index, e):
        """Adds `e` to constraint `index` (several emits of one index add up)."""
        e = e if isinstance(e, Expr) else self.const(e)
        f = self._family_of(index)
        if e.degree > f[3]:
            raise ValueError("constraint %d: degree %d, its family allows %d" % (index, e.degree, f[3]))
        if not self.units:
            self.unit()
        self.units[-1].append((index, e))

    def port(self, filter_expr, tuple_exprs):
        """A lookup port: the rows where `filter_expr` is 1 send (or expose) the tuple `tuple_exprs`.  Returns its index.
        The degrees bp_air_register asks for -- 2 deg f <= degree, 1 + deg f + max deg t <= degree, deg f + max deg t <=
        boundary_degree(degree) -- are checked by assemble(), when the program's degree is known."""
        f = filter_expr if isinstance(filter_expr, Expr) else self.const(filter_expr)
        t = [e if isinstance(e, Expr) else self.const(e) for e in tuple_exprs]
        if not 1 <= len(t) <= MAX_TUPLE:
            raise ValueError("a port's tuple has 1 .. %d elements: got %d" % (MAX_TUPLE, len(t)))
        if len(self.ports) == MAX_PORTS:
            raise ValueError("a program has at most %d ports" % MAX_PORTS)
        self.ports.append((f, t))
        self.port_kinds.append(PORT_PRODUCT)
        return len(self.ports) - 1

    def log_port(self, filter_expr, tuple_exprs, multiplicity=False):
        """A log port: the port's two running columns are sums of filter / (gamma + compressed tuple).  With
        multiplicity=False the filter is a bit (the library adds f f - f): the rows where it is 1 send the tuple.  With
        multiplicity=True the filter is any field value: the row exposes (or sends) its tuple that many times.  Returns
        the port's index.  The degrees bp_air_register asks for -- max(1 + max deg t, deg f) <= degree and <=
        boundary_degree(degree), and 2 deg f <= degree for a bit filter -- are checked by assemble()."""
        l = self.port(filter_expr, tuple_exprs)
        self.port_kinds[l] = PORT_LOG_MULT if multiplicity else PORT_LOG_BIT
        return l

    @staticmethod
    def _port_degree(kind, df, dt):
        """the degree a port's derived constraints need of the program"""
        if kind == PORT_PRODUCT:
            return max(2 * df, 1 + df + dt)
        return max(1 + dt, df, 2 * df if kind == PORT_LOG_BIT else 0)

    def _check_ports(self, degree):
        for l, (f, t) in enumerate(self.ports):
            dt = max(e.degree for e in t)
            kind = self.port_kinds[l]
            if kind != PORT_PRODUCT:
                if self._port_degree(kind, f.degree, dt) > degree or max(1 + dt, f.degree) > boundary_degree(degree):
                    raise ValueError("log port %d: a filter of degree %d and a tuple of degree %d do not fit a program of degree %d"
                                     % (l, f.degree, dt, degree))
                continue
            if 2 * f.degree > degree or 1 + f.degree + dt > degree or f.degree + dt > boundary_degree(degree):
                raise ValueError("port %d: a filter of degree %d and a tuple of degree %d do not fit a program of degree %d"
                                 % (l, f.degree, dt, degree))
        if len(self.families) > MAX_FAMILIES_WITH_PORTS:
            raise ValueError("%d families: a program with ports has at most %d of its own" % (len(self.families), MAX_FAMILIES_WITH_PORTS))

    # ---- the independent statement: the constraints over Python integers
    def _values(self, row, next_row, consts, pub, x):
        val = [None] * len(self._order)
        for e in self._order:
            if e.op == OP_LOC:
                v = int(row[e.a])
            elif e.op == OP_NXT:
                v = int(next_row[e.a])
            elif e.op == OP_CST:
                v = int(consts[e.a])
            elif e.op == OP_PUB:
                v = int(pub[e.a])
            elif e.op == OP_X:
                v = int(x)
            elif e.op == OP_IMM:
                v = e.a
            elif e.op == OP_ADD:
                v = val[e.a.n] + val[e.c.n]
            elif e.op == OP_SUB:
                v = val[e.a.n] - val[e.c.n]
            else:
                v = val[e.a.n] * val[e.c.n]
            val[e.n] = v % P
        return val

    def evaluate(self, row, next_row, consts=(), pub=(), x=0):
        """[n_constraints] values mod p at one row: row / next_row / consts / pub are sequences of integers."""
        val = self._values(row, next_row, consts, pub, x)
        out = [0] * self.n_constraints
        for u in self.units:
            for index, e in u:
                out[index] = (out[index] + val[e.n]) % P
        return out

    def evaluate_ports(self, row, next_row, consts=(), pub=(), x=0):
        """Per port (f, [t_j]) mod p at one row, over Python integers."""
        val = self._values(row, next_row, consts, pub, x)
        return [(val[f.n], [val[e.n] for e in t]) for f, t in self.ports]

    def port_running_columns(self, trace, ctl, consts=None, pub=(0, 0, 0, 0)):
        """[2 * n_ports][n] Python integers: the two running columns of every port over the trace ([n_cols][n], and consts
        [n_const][n]), as the prover's witness sees the rows (nxt wraps at the last row, x = w^i): port l's columns at 2l,
        2l + 1, column c under the challenge set (beta, gamma) = ctl[2c], ctl[2c + 1].  A product port:
        z[i] = prod_{i' >= i} (1 + f (gamma + v - 1)).  A log port: s[i] = sum_{i' >= i} f / (gamma + v), the inverse as
        pow(d, P - 2, P); a row where gamma + v = 0 contributes 0 when f = 0 and raises ValueError (a pole) otherwise."""
        n = len(trace[0])
        log_n = n.bit_length() - 1
        w = pow(7, (P - 1) >> log_n, P)
        rows = [[int(col[i]) for col in trace] for i in range(n)]
        crow = [[int(col[i]) for col in consts] for i in range(n)] if consts is not None else [()] * n
        terms = [[0] * n for _ in range(2 * len(self.ports))]
        x = 1
        for i in range(n):
            for l, (f, t) in enumerate(self.evaluate_ports(rows[i], rows[(i + 1) % n], crow[i], pub, x)):
                for c in range(2):
                    d = (ctl[2 * c + 1] + sum(pow(ctl[2 * c], j, P) * tj for j, tj in enumerate(t))) % P
                    if self.port_kinds[l] == PORT_PRODUCT:
                        terms[2 * l + c][i] = (1 + f * (d - 1)) % P
                    elif d == 0 and f != 0:
                        raise ValueError("a pole: port %d, challenge set %d, row %d" % (l, c, i))
                    else:
                        terms[2 * l + c][i] = f * pow(d, P - 2, P) % P
            x = x * w % P
        out = []
        for k, col in enumerate(terms):
            product = self.port_kinds[k // 2] == PORT_PRODUCT
            run, acc = [0] * n, 1 if product else 0
            for i in range(n - 1, -1, -1):
                acc = acc * col[i] % P if product else (acc + col[i]) % P
                run[i] = acc
            out.append(run)
        return out

    # ---- the words
    def _schedule(self, emits):
        """The unit as a list of steps ('node', Expr) / ('emit', index, Expr) / ('drop', leaves): every operand before
        its user, a non-leaf node once per unit, a leaf once per emit."""
        steps, done = [], set()
        for index, root in emits:
            leaves = set()
            stack = [(root, False)]
            while stack:
                e, expanded = stack.pop()
                if e.n in done or e.n in leaves:
                    continue
                if e.op in _LEAVES:
                    leaves.add(e.n)
                    steps.append(("node", e))
                elif expanded:
                    done.add(e.n)
                    steps.append(("node", e))
                else:
                    stack.append((e, True))
                    stack.append((e.c, False))
                    stack.append((e.a, False))
            steps.append(("emit", index, root))
            # a leaf scheduled for this emit lives until its last use in it: later emits load it again
            steps.append(("drop", leaves))
        return steps

    def _assemble_unit(self, emits, port=None):
        """port: None for a constraint unit; else the unit of that port, whose `emits` are (slot, Expr)."""
        steps = self._schedule(emits)
        # last use of every value instance; a dropped leaf's next load is a new instance
        inst, cur = [], {}   # step number -> instance id of the node it defines; node -> live instance
        last_use = {}
        uses = []            # per step: instance ids it reads
        n_inst = 0
        for i, s in enumerate(steps):
            if s[0] == "node":
                e = s[1]
                reads = [] if e.op in _LEAVES else [cur[e.a.n], cur[e.c.n]]
                cur[e.n] = n_inst
                inst.append(n_inst)
                n_inst += 1
            elif s[0] == "emit":
                reads = [cur[s[2].n]]
                inst.append(None)
            else:
                for n in s[1]:
                    cur.pop(n, None)
                reads = []
                inst.append(None)
            for r in reads:
                last_use[r] = i
            uses.append(reads)
        free, reg, words, top = [], {}, [], 0
        for i, s in enumerate(steps):
            if s[0] == "drop":
                continue
            regs = [reg[r] for r in uses[i]]
            for r in set(uses[i]):
                if last_use[r] == i:
                    free.append(reg.pop(r))
            if s[0] == "emit":
                if port is None:
                    words.append(OP_EMIT | self._family_of(s[1])[2] << 8 | s[1] << 16 | regs[0] << 40)
                else:
                    words.append(OP_PORT | s[1] << 8 | port << 16 | regs[0] << 40)
                continue
            e, me = s[1], inst[i]
            if me not in last_use:
                raise AssertionError("a value nobody reads was scheduled")
            free.sort()
            d = free.pop(0) if free else top
            top = max(top, d + 1)
            reg[me] = d
            if e.op == OP_IMM:
                words += [OP_IMM | d << 8, e.a]
            elif e.op == OP_X:
                words.append(OP_X | d << 8)
            elif e.op in _LEAVES:
                words.append(e.op | d << 8 | e.a << 16)
            else:
                words.append(e.op | d << 8 | regs[0] << 16 | regs[1] << 40)
        return words, top

    def assemble(self, check_ports=True):
        """The program as numpy uint64 words (bp_air_register's input): "BPGAIRP1"; "BPGAIRP2" when the builder has a
        port; "BPGAIRP3" only when one of them is a log port, so programs that existed before keep their bytes.
        check_ports=False leaves the ports' degree rules to bp_air_register (the tests of its refusals)."""
        if not self.families or not self.units:
            raise ValueError("a program has at least one family and one unit")
        code, offsets, n_regs = [], [0], 1
        for u in self.units:
            words, top = self._assemble_unit(u)
            code += words
            offsets.append(len(code))
            n_regs = max(n_regs, top)
        for l, (f, t) in enumerate(self.ports):
            words, top = self._assemble_unit([(0, f)] + [(1 + j, e) for j, e in enumerate(t)], port=l)
            code += words
            offsets.append(len(code))
            n_regs = max(n_regs, top)
        if n_regs > MAX_REGS:
            raise ValueError("the program needs %d registers, the library takes %d: split the unit" % (n_regs, MAX_REGS))
        # the declared degree, else what the families and the ports' derived constraints (f f - f, z - z' term;
        # (s - s') d - f) need
        degree = self.degree if self.degree is not None else max(
            [f[3] for f in self.families] + [self._port_degree(kind, f.degree, max(e.degree for e in t))
                                             for (f, t), kind in zip(self.ports, self.port_kinds)])
        for f in self.families:
            self._check_boundary(f[2], f[3], degree)
        hdr = [MAGIC, self.n_cols, self.n_const, self.n_public, degree, self.n_constraints, len(self.families), n_regs,
               len(self.units), len(code)]
        fam = [w for f in self.families for w in f]
        if self.ports:
            if check_ports:
                self._check_ports(degree)
            hdr = [MAGIC3 if any(self.port_kinds) else MAGIC2] + hdr[1:] + [len(self.ports)]
            fam += [len(t) | kind << 32 for (_, t), kind in zip(self.ports, self.port_kinds)]
        return np.array(hdr + fam + offsets + code, dtype=np.uint64)
