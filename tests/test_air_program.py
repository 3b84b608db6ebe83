"""Run-time AIRs on the CPU (csrc/air_program.hpp / air_program.cpp, proof_protocol_decoder_amd/air_program.py): the
validator and the registry, bp_air_describe of a registered id, the host interpreter against the builder's evaluate()
over Python integers and against the built-in AIRs 3, 4 and 7 it transcribes (tests/air_program_cases.py), the CPU
verifier on oracle proofs under a registered id, and the new device source under the rules tests/test_build.py applies
to the kernel sources.  Everything is exact.  GPU side: tests/test_gpu_air_program.py."""
import re

import numpy as np
import pytest

import air_program_cases as cases
import air_program_random as rnd
import builtin_airs as ba
from air_program_cases import P
from proof_protocol_decoder_amd.air_program import (ALL_ROWS, FIRST_ROW, LAST_ROW, OP_EMIT, OP_IMM, OP_LOC, OP_MUL, TRANSITION,
                                                    Builder)
from util import rand_field


def ops():
    import proof_protocol_decoder_amd as pkg
    pkg.lib()
    return pkg.ops


def keccak256(data):
    """Keccak-256 from the specification (FIPS 202 with the 0x01 padding byte), on Python integers"""
    rc, r = [], 1
    for _ in range(24):
        c = 0
        for j in range(7):
            if r & 1:
                c |= 1 << ((1 << j) - 1)
            r = ((r << 1) ^ (0x71 if r & 0x80 else 0)) & 0xFF
        rc.append(c)
    rot = lambda v, n: ((v << n) | (v >> (64 - n))) & (2 ** 64 - 1) if n else v
    pad = 136 - len(data) % 136
    msg = bytes(data) + (b"\x81" if pad == 1 else b"\x01" + b"\x00" * (pad - 2) + b"\x80")
    a = [0] * 25
    for off in range(0, len(msg), 136):
        for i in range(17):
            a[i] ^= int.from_bytes(msg[off + 8 * i:off + 8 * i + 8], "little")
        for rnd in range(24):
            c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
            d = [c[(x - 1) % 5] ^ rot(c[(x + 1) % 5], 1) for x in range(5)]
            a = [a[i] ^ d[i % 5] for i in range(25)]
            b, x, y = [0] * 25, 1, 0
            b[0] = a[0]
            for t in range(24):
                b[y + 5 * ((2 * x + 3 * y) % 5)] = rot(a[x + 5 * y], ((t + 1) * (t + 2) // 2) % 64)
                x, y = y, (2 * x + 3 * y) % 5
            a = [b[i] ^ (~b[(i % 5 + 1) % 5 + 5 * (i // 5)] & b[(i % 5 + 2) % 5 + 5 * (i // 5)]) for i in range(25)]
            a[0] ^= rc[rnd]
    return b"".join(v.to_bytes(8, "little") for v in a[:4])


# ---------------------------------------------------------------------------------------------- 1. validator, registry


def tiny():
    b = Builder(8, n_const=1, n_public=1)
    f0 = b.family(2, ALL_ROWS, 2)
    f1 = b.family(1, TRANSITION, 1)
    b.unit()
    b.emit(f0, b.loc(0) * b.loc(1) - 3 * b.loc(2))
    b.emit(f0 + 1, b.cst(0) * b.loc(3) - b.pub(0))
    b.unit()
    b.emit(f1, b.nxt(0) - b.loc(0))
    return b.assemble()


HDR, N_FAM, N_UNITS = 10, 2, 2
FAM0, OFF0 = HDR, HDR + 4 * N_FAM
CODE0 = OFF0 + N_UNITS + 1


def code_words(w):
    """[(word offset, op, dst, a, b)] of the program's instructions (an imm's constant word is skipped)"""
    out, pc = [], CODE0
    while pc < len(w):
        c = int(w[pc])
        out.append((pc, c & 0xFF, (c >> 8) & 0xFF, (c >> 16) & 0xFFFFFF, c >> 40))
        pc += 2 if c & 0xFF == OP_IMM else 1
    return out


def first_op(w, op, nth=0):
    return [i for i in code_words(w) if i[1] == op][nth]


def set_field(w, off, shift, bits, value):
    w[off] = np.uint64((int(w[off]) & ~(((1 << bits) - 1) << shift)) | (value << shift))


def _bad_magic(w):
    w[0] ^= np.uint64(1)
    return 0


def _too_many_regs(w):
    w[7] = 65
    return 7


def _wrong_length(w):
    w[9] += np.uint64(1)
    return 9


def _read_before_write(w):
    w[7] = 10                                   # registers 0 .. 9 exist, nothing writes register 9
    off = first_op(w, OP_MUL)[0]
    set_field(w, off, 16, 24, 9)
    return off


def _column_out_of_range(w):
    off = first_op(w, OP_LOC)[0]
    set_field(w, off, 16, 24, 8)
    return off


def _register_out_of_range(w):
    off = first_op(w, OP_LOC)[0]
    set_field(w, off, 8, 8, int(w[7]))
    return off


def _constraint_out_of_range(w):
    off = first_op(w, OP_EMIT)[0]
    set_field(w, off, 16, 24, 3)
    return off


def _non_canonical_immediate(w):
    off = first_op(w, OP_IMM)[0]
    w[off + 1] = P
    return off + 1


def _never_emitted(w):
    off = first_op(w, OP_EMIT, 1)[0]            # constraint 1 is emitted into constraint 0 instead
    set_field(w, off, 16, 24, 0)
    return FAM0


def _families_do_not_tile(w):
    w[FAM0 + 4] += np.uint64(1)
    return FAM0 + 4


def _families_end_short(w):
    w[5] += np.uint64(1)                        # one more constraint than the families cover
    return FAM0 + 4 + 1


def _emit_degree(w):
    w[FAM0 + 3] = 1                             # family 0 now allows degree 1; its first emit is a product
    return first_op(w, OP_EMIT)[0]


def _family_degree(w):
    w[4] = 1                                    # the program's degree below family 0's
    return FAM0 + 3


def _emit_kind(w):
    off = first_op(w, OP_EMIT)[0]
    set_field(w, off, 8, 8, 1)
    return off


def _unit_table(w):
    w[OFF0 + 1] = w[OFF0 + 2] + np.uint64(1)
    return OFF0 + 1


def _boundary_family_degree(w):
    w[4] = 3                                    # a degree-3 program whose family 1 is a first-row family of degree 3
    w[FAM0 + 4 + 2], w[FAM0 + 4 + 3] = 2, 3
    return FAM0 + 4 + 3


RULES = [_boundary_family_degree, _bad_magic, _too_many_regs, _wrong_length, _read_before_write, _column_out_of_range, _register_out_of_range,
         _constraint_out_of_range, _non_canonical_immediate, _never_emitted, _families_do_not_tile, _families_end_short,
         _emit_degree, _family_degree, _emit_kind, _unit_table]


@pytest.mark.parametrize("rule", RULES, ids=[r.__name__[1:] for r in RULES])
def test_validator_refuses_and_names_the_word(rule):
    from proof_protocol_decoder_amd._lib import BpgError
    w = tiny()
    ops().air_unregister(ops().air_register(w))          # the program itself is fine
    off = rule(w)
    with pytest.raises(BpgError) as e:
        ops().air_register(w)
    assert e.value.code == -2 and re.search(r"word %d\b" % off, e.value.message), e.value.message


def test_degree_violation_says_so():
    from proof_protocol_decoder_amd._lib import BpgError
    w = tiny()
    _emit_degree(w)
    with pytest.raises(BpgError, match="degree violation"):
        ops().air_register(w)


def test_ids_are_the_keccak_rule_and_registering_twice_gives_one_id():
    import proof_protocol_decoder_amd as pkg
    from proof_protocol_decoder_amd import compact
    from proof_protocol_decoder_amd._lib import BpgError
    o = ops()
    assert keccak256(b"") == bytes.fromhex("c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470")
    w = tiny()
    raw = w.astype("<u8").tobytes()
    digest = keccak256(raw)
    assert digest == compact.keccak256(raw)
    want = 0x80000000 | (int.from_bytes(digest[:4], "little") & 0x7FFFFFFF)
    a, b = o.air_register(w), o.air_register(w.copy())
    assert a == b == want and o.air_program_digest(a) == digest
    assert pkg.lib().bp_air_count() == 9
    other = cases.register(cases.fibonacci_program())
    assert other != a and pkg.lib().bp_air_count() == 9
    o.air_unregister(a)
    with pytest.raises(BpgError):
        o.air_program_digest(a)
    with pytest.raises(BpgError):
        o.air_unregister(a)
    with pytest.raises(BpgError, match="unknown air_id"):
        o.check_air_trace_host(a, np.zeros((8, 16), dtype=np.uint64))
    assert o.air_register(w) == want


def test_a_registered_air_cannot_be_proven_from_a_seed():
    from proof_protocol_decoder_amd._lib import BpgError
    air = cases.register(cases.arithmetic_program())
    with pytest.raises(BpgError, match="bp_stark_prove_trace"):
        ops().stark_prove_air(air, cases.cfg_for(air, 5, num_queries=6, pow_bits=6), 1)


# ---------------------------------------------------------------------------------------------- 2. describe

TRANSCRIPTIONS = {3: cases.memory_program, 4: cases.arithmetic_program, 7: cases.arithmetic_mul_program}


@pytest.mark.parametrize("air_id", sorted(TRANSCRIPTIONS))
def test_describe_of_a_transcription_has_the_built_ins_shape(air_id):
    o = ops()
    reg = cases.register(TRANSCRIPTIONS[air_id]())
    d, want = o.air_describe(reg), o.air_describe(air_id)
    assert d.air_id == reg and reg & 0x80000000
    for field in ("fixed_n_cols", "n_cols", "n_const_max", "degree", "n_air_constraints", "n_units"):
        assert getattr(d, field) == getattr(want, field), field
    assert (d.n_aux, d.n_ctl_constraints) == (1, 2)          # "a table no lookup is built for"
    fams = lambda x: [(f.first_index, f.count, f.kind, f.degree) for f in x.families[:x.n_families]]
    own = len(cases.own_families(air_id))
    assert fams(d)[:own] == fams(want)[:own]
    assert fams(d)[own:] == [(d.n_air_constraints, 1, 1, 3), (d.n_air_constraints + 1, 1, 3, 2)]
    if air_id != 3:                                          # AIR 4 and AIR 7 have exactly that auxiliary column
        assert fams(d) == fams(want) and (want.n_aux, want.n_ctl_constraints) == (1, 2)


# ---------------------------------------------------------------------------------------------- 3. against Python integers


def active(kind, i, n):
    return kind == 0 or (kind == 1 and i != n - 1) or (kind == 2 and i == 0) or (kind == 3 and i == n - 1)


def expected_violations(b, trace, consts=None, pub=(0, 0, 0, 0)):
    """(row, constraint, family, kind, value) of every non-zero constraint the trace domain's selectors leave on, from
    Builder.evaluate over Python integers"""
    n = trace.shape[1]
    log_n = n.bit_length() - 1
    w = pow(7, (P - 1) >> log_n, P)
    out = []
    for i in range(n):
        vals = b.evaluate(trace[:, i], trace[:, (i + 1) % n], consts[:, i] if consts is not None else (), pub, pow(w, i, P))
        for fi, (first, count, kind, _) in enumerate(b.families):
            if active(kind, i, n):
                out += [(i, first + j, fi, kind, vals[first + j]) for j in range(count) if vals[first + j]]
    return out


def reported(r):
    return [(v.row, v.constraint, v.family, v.kind, v.value) for v in r.violations]


@pytest.mark.parametrize("name", ["memory", "arithmetic", "arithmetic_mul", "fibonacci"])
def test_host_interpreter_gives_the_values_of_python_integers(name):
    """Seeded random rows (no witness: every constraint is non-zero): per row and constraint index the host checker on
    the registered id reports what evaluate() computes."""
    b = getattr(cases, name + "_program")()
    air = cases.register(b)
    rng = np.random.default_rng(len(name))
    n = 16
    trace = rand_field(rng, (b.n_cols, n))
    consts = rand_field(rng, (b.n_const, n)) if b.n_const else None
    pub = [int(v) for v in rand_field(rng, (4,), edge=False)] if b.n_public else None
    want = expected_violations(b, trace, consts, pub or (0, 0, 0, 0))
    assert len(want) > (n - 1) * b.n_constraints * 3 // 4
    r = ops().check_air_trace_host(air, trace, consts=consts, pub=pub, max_rows=n, max_viol=len(want) + 8)
    assert r.n_violated_rows == n and r.rows == list(range(n)) and r.n_violations == len(want)
    assert reported(r) == want


# ---------------------------------------------------------------------------------------------- 3b. random programs


@pytest.mark.parametrize("name", rnd.CASES + rnd.PROBES)
def test_a_random_program_is_what_its_case_says(name):
    """the generator's own assertions (air_program_random.check_program and case): degree, units, registers, every
    operation, kind, input and edge immediate, an index fed from two units"""
    c = rnd.case(name)
    assert c.n_constraints == c.b.n_constraints and c.b.n_cols == c.n_free + c.n_constraints


@pytest.mark.parametrize("name", rnd.CASES)
def test_host_checker_on_random_rows_of_a_random_program(name):
    """32 random rows (nothing is satisfied): the host checker reports evaluate()'s values, tuple for tuple"""
    c = rnd.case(name)
    air = ops().air_register(c.words)
    rng = np.random.default_rng([7, c.kw["seed"]])
    n = 32
    trace = rand_field(rng, (c.b.n_cols, n))
    consts = rand_field(rng, (c.b.n_const, n))
    pub = [int(v) for v in rand_field(rng, (4,), edge=False)]
    want = expected_violations(c.b, trace, consts, pub)
    assert len(want) > c.n_constraints                       # (first-row and last-row families count once)
    r = ops().check_air_trace_host(air, trace, consts=consts, pub=pub, max_rows=n, max_viol=len(want) + 8)
    assert r.n_violated_rows == n and r.rows == list(range(n)) and r.n_violations == len(want)
    assert reported(r) == want


@pytest.mark.parametrize("log_n", [5, 8])
@pytest.mark.parametrize("name", rnd.CASES)
def test_host_checker_accepts_the_constructed_witness(name, log_n):
    """the witness is valid although every slack cell is wrong where its constraint's kind is switched off: a selector
    that masked nothing would report those rows"""
    c = rnd.case(name)
    air = ops().air_register(c.words)
    trace, consts, pub = rnd.witness(name, log_n)
    r = ops().check_air_trace_host(air, trace, consts=consts, pub=pub)
    assert r.ok and r.rows == [] and r.violations == [] and r.n_violations == 0, r


@pytest.mark.parametrize("name", rnd.CASES)
def test_a_corrupted_cell_of_a_random_program_is_reported_as_python_computes_it(name):
    """one slack cell per kind on a row where the kind is on, and one free cell that a nxt reads (the violation lands
    on the row before as well): (row, constraint, family, kind, value) are evaluate()'s"""
    c = rnd.case(name)
    air = ops().air_register(c.words)
    clean, consts, pub = rnd.witness(name, 5)
    n = clean.shape[1]
    rng = np.random.default_rng([11, c.kw["seed"]])
    bump = lambda t, col, row: (int(t[col, row]) + 1 + int(rng.integers(0, 1 << 40))) % P
    for kind in rnd.KINDS:                                   # the slack cell's own constraint, on its own row, only
        row, col = rnd.active_cell(c, kind, n, rng)
        t = clean.copy()
        t[col, row] = bump(t, col, row)
        want = expected_violations(c.b, t, consts, pub)
        assert [(v[0], v[1], v[3]) for v in want] == [(row, col - c.n_free, kind)], want
        _same_report(air, t, consts, pub, want)
    for row in (9, 0):                                       # a free cell some nxt reads: row 0's readers sit on row n - 1
        for col in range(c.n_free):
            t = clean.copy()
            t[col, row] = bump(t, col, row)
            want = expected_violations(c.b, t, consts, pub)
            if (row - 1) % n in {v[0] for v in want}:
                break
        else:
            raise AssertionError("no free column of row %d is read as a next row" % row)
        _same_report(air, t, consts, pub, want)


def _same_report(air, t, consts, pub, want):
    n = t.shape[1]
    r = ops().check_air_trace_host(air, t, consts=consts, pub=pub, max_rows=n, max_viol=len(want) + 8)
    assert reported(r) == want and r.n_violations == len(want)
    assert r.rows == sorted({v[0] for v in want}) and r.n_violated_rows == len(r.rows)


@pytest.mark.parametrize("name", rnd.PROBES)
def test_a_first_row_or_last_row_family_above_its_degree_cap_is_refused(name):
    """A program of degree 3 whose first-row and last-row families are cubic, and one of degree 9 with families of degree
    9.  The validator used to register both.  The selector of such a row is a Lagrange polynomial of degree n - 1: a
    family of degree d leaves a quotient of degree (d + 1)(n - 1) - n, and the 2^rate_bits n quotient coefficients hold
    that only for d <= 2^rate_bits (the test below computes 92 against 64 and 278 against 256 at 2^5 rows), so an honest
    proof cannot pass the constraint check at zeta; with those families at degree 2 / 8 the generator's programs prove
    and verify (tests/test_gpu_air_program.py).  So the validator refuses the program and names the family's degree
    word, and the builder raises on the same condition."""
    from proof_protocol_decoder_amd._lib import BpgError
    c = rnd.case(name)
    above = [(k, f) for k, f in enumerate(c.b.families) if f[2] >= 2]
    assert above and all(f[3] == c.degree > rnd.boundary_degree_cap(c.degree) for _, f in above)
    with pytest.raises(BpgError) as e:
        ops().air_register(c.words)
    assert e.value.code == -2 and re.search(r"word %d: family %d: a (first|last)-row family of degree %d" % (
        10 + 4 * above[0][0] + 3, above[0][0], c.degree), e.value.message), e.value.message
    w = c.words.copy()                                       # at the cap the same words register
    for k, _ in above:
        w[10 + 4 * k + 3] = rnd.boundary_degree_cap(c.degree)
    with pytest.raises(BpgError, match="degree violation"):  # (the emits are still cubic)
        ops().air_register(w)
    for kind in (FIRST_ROW, LAST_ROW):
        with pytest.raises(ValueError, match="first-row or last-row"):
            Builder(8, degree=c.degree).family(1, kind, c.degree)
        assert Builder(8, degree=c.degree).family(1, kind, rnd.boundary_degree_cap(c.degree)) == 0
    late = Builder(8)                                        # no declared degree: the families' maximum, known at assemble()
    late.emit(late.family(1, FIRST_ROW, 3), late.loc(0) * late.loc(1) * late.loc(2))
    with pytest.raises(ValueError, match="first-row or last-row"):
        late.assemble()


@pytest.mark.parametrize("above,at_cap", [("first-row-deg3", "deg3-u5"), ("first-row-deg9", "deg9-u5")])
def test_the_honest_quotient_of_a_boundary_family_above_its_cap_does_not_fit_the_proof(above, at_cap):
    """why the rule: over Python integers at 2^5 rows, the quotient of a valid witness has degree (d + 1)(n - 1) - n for
    first-row and last-row families of degree d -- past the n << rate_bits coefficients a proof holds when d is the
    program's degree, within them at the cap"""
    n = 32
    for name, fits in ((above, False), (at_cap, True)):
        c = rnd.case(name)
        d = max(f[3] for f in c.b.families if f[2] >= 2)
        assert d == (rnd.boundary_degree_cap(c.degree) if fits else c.degree)
        degree = rnd.honest_quotient_degree(name)
        assert degree == (d + 1) * (n - 1) - n and (degree < n << c.rate_bits) == fits, (name, degree)


# ---------------------------------------------------------------------------------------------- 3c. the validator, restated

MAGIC = int.from_bytes(b"BPGAIRP1", "little")


def restated_accepts(words):
    """include/bpg.h's "Run-time AIRs" comment as code, written from that text (not from csrc/air_program.cpp): True
    where the comment says bp_air_register takes the words"""
    w = [int(v) for v in words]
    if len(w) < 10 or w[0] != MAGIC:
        return False
    limits = [(8, 65536), (0, 4096), (0, 4), (1, 9), (1, 65536), (1, 24), (1, 64), (1, 256), (1, 1 << 20)]
    if any(not lo <= v <= hi for v, (lo, hi) in zip(w[1:10], limits)):
        return False
    n_cols, n_const, n_public, degree, n_constraints, n_families, n_regs, n_units, n_code = w[1:10]
    off0 = 10 + 4 * n_families
    code0 = off0 + n_units + 1
    if len(w) != code0 + n_code:
        return False
    family_of, covered = [], 0
    for f in range(n_families):
        first, count, kind, deg = w[10 + 4 * f:14 + 4 * f]
        if first != covered or count < 1 or covered + count > n_constraints:        # in order, exactly once
            return False
        if kind > 3 or not 1 <= deg <= degree:
            return False
        if kind >= 2 and deg > (2 if degree <= 3 else 8):                            # first row, last row
            return False
        family_of += [(kind, deg)] * count
        covered += count
    if covered != n_constraints:
        return False
    off = w[off0:code0]
    if off[0] != 0 or off[n_units] != n_code or any(off[u + 1] <= off[u] for u in range(n_units)):
        return False
    emitted = set()
    for u in range(n_units):
        deg_of = {}                                                                  # registers do not live across units
        pc, end = code0 + off[u], code0 + off[u + 1]
        while pc < end:
            op, dst, a, b = w[pc] & 0xFF, (w[pc] >> 8) & 0xFF, (w[pc] >> 16) & 0xFFFFFF, w[pc] >> 40
            pc += 1
            if op > 9:
                return False
            if op == 9:
                if a >= n_constraints or b not in deg_of or dst != family_of[a][0] or deg_of[b] > family_of[a][1]:
                    return False
                emitted.add(a)
                continue
            if dst >= n_regs:
                return False
            if op in (0, 1):
                ok, d = a < n_cols, 1
            elif op == 2:
                ok, d = a < n_const, 1
            elif op == 3:
                ok, d = a < n_public, 0
            elif op == 4:
                ok, d = True, 1
            elif op == 5:
                ok, d = pc < end and w[pc] < P, 0
                pc += 1
            else:
                ok = a in deg_of and b in deg_of                                     # (a register >= n_regs is never written)
                d = ok and (deg_of[a] + deg_of[b] if op == 8 else max(deg_of[a], deg_of[b]))
            if not ok:
                return False
            deg_of[dst] = d
    return len(emitted) == n_constraints


def mutants(words, rng, count):
    """`count` single-word mutations of a program: (offset, value), the value another than the word's"""
    h = rnd.header(words)
    off0 = 10 + 4 * h["n_families"]
    code0 = off0 + h["n_units"] + 1
    regions = [(0, 10), (10, off0), (off0, code0), (code0, len(words))]
    edges = [0, 1, P - 1, P, P + 1, (1 << 32) - 1, 1 << 32, (1 << 64) - 1, 1 << 63]
    out = []
    while len(out) < count:
        lo, hi = regions[int(rng.choice(4, p=[0.1, 0.15, 0.05, 0.7]))]
        at = int(rng.integers(lo, hi))
        old = int(words[at])
        how = int(rng.integers(0, 8))
        if how == 0:
            new = int(rng.integers(0, 70))
        elif how == 1:
            new = edges[int(rng.integers(0, len(edges)))]
        elif how == 2:
            new = int(words[int(rng.integers(0, len(words)))])
        elif how == 3:                                       # a word of the same region: a family field, another instruction
            new = int(words[int(rng.integers(lo, hi))])
        elif how == 4:                                       # a small step: the next column, register, count
            new = (old + int(rng.choice([-1, 1])) * (1 << int(rng.choice([0, 8, 16, 40])))) % (1 << 64)
        else:
            new = old ^ (1 << int(rng.integers(0, 64)))
        if new != old:
            out.append((at, new))
    return out


def test_validator_accepts_exactly_what_the_header_comment_says():
    """2100 seeded single-word mutations of three random programs (header, family, offset and code words; small
    integers, the field's edges, bit flips, other words of the program): bp_air_register takes exactly the mutants the
    restatement of include/bpg.h takes.  At least a quarter are taken and a quarter refused, by the restatement alone."""
    from proof_protocol_decoder_amd._lib import BpgError
    o = ops()
    taken = refused = 0
    for name in ("deg3-u5", "inputs", "regs-mid"):
        words = rnd.case(name).words
        assert restated_accepts(words)
        rng = np.random.default_rng([13, rnd.case(name).kw["seed"]])
        for at, new in mutants(words, rng, 700):
            w = words.copy()
            w[at] = np.uint64(new)
            want = restated_accepts(w)
            taken, refused = taken + want, refused + (not want)
            try:
                air = o.air_register(w)
            except BpgError as e:
                assert e.code == -2 and re.search(r"word \d+: ", e.message), e.message
                assert not want, "%s: word %d = 0x%x is refused (%s); include/bpg.h takes it" % (name, at, new, e.message)
            else:
                o.air_unregister(air)
                assert want, "%s: word %d = 0x%x is registered; include/bpg.h refuses it" % (name, at, new)
    assert taken + refused == 2100 and 4 * taken >= 2100 and 4 * refused >= 2100, (taken, refused)


# ---------------------------------------------------------------------------------------------- 4. against the built-ins

@pytest.mark.parametrize("air_id", sorted(TRANSCRIPTIONS))
def test_a_valid_witness_has_no_violation_under_its_transcription(oracle, air_id):
    reg = cases.register(TRANSCRIPTIONS[air_id]())
    for seed in (1, 0xC0DE):
        r = ops().check_air_trace_host(reg, oracle.air_trace(air_id, 6, seed=seed))
        assert r.ok and r.rows == [] and r.violations == [], r


def _breaks():
    return [b[:4] for b in ba.checker_breaks() if b[0] in TRANSCRIPTIONS]


def both_checks(reg, air_id, t):
    got = ops().check_air_trace_host(reg, t, max_rows=64, max_viol=4096)
    want = ops().check_air_trace_host(air_id, t, max_rows=64, max_viol=4096)
    assert want.n_violated_rows >= 1
    assert (got.n_violated_rows, got.rows, got.n_violations) == (want.n_violated_rows, want.rows, want.n_violations)
    assert reported(got) == reported(want)
    return got


@pytest.mark.parametrize("air_id,col,row,val", _breaks(), ids=["%d-col%d@%d" % b[:3] for b in _breaks()])
def test_a_corrupted_cell_gives_the_built_ins_violations(oracle, air_id, col, row, val):
    """one cell per constraint family (the cells tests/test_air_check.py breaks): the same (row, constraint, family,
    kind, value) list from the transcription and from the built-in id"""
    reg = cases.register(TRANSCRIPTIONS[air_id]())
    t = oracle.air_trace(air_id, 6, seed=0xC0DE)
    t[col, row] = np.uint64(val) if val is not None else t[col, row] ^ np.uint64(1)
    both_checks(reg, air_id, t)


def test_the_memory_airs_value_families_give_the_built_ins_violations(oracle):
    """AIR 3's M5 (a stale read), M6 (a first read that is not zero) and M7 (a read in the first row), which the cell
    list above leaves to log-level tests: the rows are picked from the trace"""
    reg = cases.register(cases.memory_program())
    clean = oracle.memory_trace(6, seed=0xC0DE)
    rd, chg = clean[0], clean[11]
    stale = next(i for i in range(1, 63) if rd[i] == 1 and chg[i - 1] == 0)
    fresh = next(i for i in range(1, 63) if chg[i - 1] == 1)
    seen = set()
    for cells in ([(3 + 2, stale, int(clean[3 + 2, stale]) ^ 5)], [(0, fresh, 1), (3 + 4, fresh, 7)], [(0, 0, 1), (3, 0, 9)]):
        t = clean.copy()
        for col, row, val in cells:
            t[col, row] = np.uint64(val)
        seen |= {(v.family, v.kind) for v in both_checks(reg, 3, t).violations}
    assert {(5, 1), (6, 1), (7, 2)} <= seen, seen


# ---------------------------------------------------------------------------------------------- 5. the verifier


@pytest.mark.parametrize("air_id,log_n", [(4, 5), (4, 8), (7, 5)])
def test_oracle_proof_verifies_under_the_registered_id(oracle, air_id, log_n):
    """An oracle proof of the built-in AIR, header word 14 rewritten to the registered id (the id is in no transcript),
    is accepted under the transcription and rejected under a transcription with 65536 -> 65535 in the carry equations."""
    make = TRANSCRIPTIONS[air_id]
    cfg = ba.small_cfg(oracle, ba.AIRS[air_id], log_n)
    trace = oracle.air_trace(air_id, log_n, seed=0xA11CE + log_n)
    proof, _, _ = ba.prove(oracle, cfg, trace)
    assert int(proof[14]) == air_id
    good, wrong = cases.register(make()), cases.register(make(carry_weight=65535))
    assert good != wrong
    pc = ops().stark_cfg(cfg.log_n, cfg.n_cols, n_const=cfg.n_const, deg_pow=cfg.deg_pow, rate_bits=cfg.rate_bits,
                         cap_height=cfg.cap_height, num_queries=cfg.num_queries, pow_bits=cfg.pow_bits,
                         arity_bits=cfg.arity_bits, final_poly_bits=cfg.final_poly_bits)
    assert cases.verify(air_id, pc, proof) == 0
    assert cases.verify(good, pc, proof) == -5               # the header still names the built-in
    proof[14] = good
    assert cases.verify(good, pc, proof) == 0
    assert cases.verify(air_id, pc, proof) == -5
    proof[14] = wrong
    assert cases.verify(wrong, pc, proof) == -5
    import proof_protocol_decoder_amd as pkg
    assert b"constraint check at zeta" in pkg.lib().bp_last_error()
    bad = proof.copy()
    bad[14] = good
    bad[proof.size // 2] ^= np.uint64(1 << 9)
    assert cases.verify(good, pc, bad) == -5


# ---------------------------------------------------------------------------------------------- 6. the device source


def test_program_kernels_have_no_scratch_and_no_sgpr_spills_beyond_k5s(tmp_path):
    from test_build import device_assembly
    name, seen = None, set()
    for line in device_assembly("air_program.hip", tmp_path).splitlines():
        m = re.match(r"\s+\.name:\s+(\S+)", line)
        if m:
            name = m.group(1)
            seen.add(name)
        m = re.match(r"\s+\.private_segment_fixed_size:\s+(\d+)", line)
        if m:
            assert int(m.group(1)) == 0, (name, "scratch")
        m = re.match(r"\s+\.sgpr_spill_count:\s+(\d+)", line)
        if m:   # what tests/test_build.py allows quotient_air_kernel: kernel arguments and wave-uniform offsets
            assert int(m.group(1)) <= 40, (name, int(m.group(1)))
        m = re.match(r"\s+\.vgpr_spill_count:\s+(\d+)", line)
        if m:
            assert int(m.group(1)) == 0, (name, "vgpr spills")
    assert any("quotient_program_kernel" in s for s in seen) and any("air_check_program_kernel" in s for s in seen), seen


def test_program_kernels_have_no_carry_mask_hazard(tmp_path):
    from test_build import device_assembly, scan_carry_mask_hazards
    bad, n = scan_carry_mask_hazards(device_assembly("air_program.hip", tmp_path))
    assert n > 100 and not bad, bad[:10]


def test_program_kernels_read_their_code_with_scalar_loads_and_keep_registers_in_lds(tmp_path):
    """the instruction stream is wave-uniform (no per-lane decode) and the register file is LDS, not scratch"""
    from test_build import device_assembly
    asm = device_assembly("air_program.hip", tmp_path)
    assert "ds_read_b64" in asm and "ds_write_b64" in asm and "scratch_" not in asm
    assert len(re.findall(r"\bs_load_dwordx2\b", asm)) >= 4


def test_program_kernels_have_no_dpp_read_of_a_fresh_asm_result(tmp_path):
    """test_build.test_no_dpp_reads_a_fresh_asm_result's rule: the new file has no DPP / permlane instruction at all"""
    from test_build import device_assembly
    for line in device_assembly("air_program.hip", tmp_path).splitlines():
        t = line.strip()
        if t and not t.startswith((";", ".", "//")):
            op = t.split()[0]
            assert "_dpp" not in op and not op.startswith("v_permlane") and "quad_perm" not in t and " row_" not in t, t
