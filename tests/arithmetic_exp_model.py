"""An independent model of the exponentiation table (proof_protocol_decoder_amd/arithmetic_exp.py, csrc/
arithmetic_exp.hip), shared by tests/test_arithmetic_exp.py and tests/test_gpu_arithmetic_exp.py.  It works from the
statement in include/bpg.h and the column list in AIRS.md section 2 ("Exponentiation (a shipped program)") over Python
integers: it imports nothing of the package, so the column numbers below are a third statement of the map and the
constraints in violations() a second statement of the program; the tests compare both with the package's.  Unlike the
other tables' models this one is a model of TRACES: an operation is a chain of rows, and a forgery may touch two.

    trace_of(ops, log_n)              [2003, 2^log_n] uint64: the model trace of a list of (op, base, exponent, exposed)
    violations(trace)                 [(row, family, constraint index)]: the constraints stated here that do not vanish
    CATALOGUE                         wrong witnesses on the 2^5-row trace of small_ops(): (name, forge, {(row, family)})
"""
import random

import numpy as np

P = 2 ** 64 - 2 ** 32 + 1
B = 1 << 16
M256 = (1 << 256) - 1
NONE, EXP = 0, 1
LIVE = (EXP,)
CARRY_BITS = 20

# AIRS.md section 2: three flags, five limb blocks, five bit blocks, twice sixteen carries of 20 bits
G, FIRST, LAST = 0, 1, 2
P_, E, RES, R, OUT = 3, 19, 35, 51, 67
P_BITS, R_BITS, E_BITS, M_BITS, S_BITS = 83, 339, 595, 851, 1107
M_CARRY, S_CARRY, N_COLS = 1363, 1683, 2003
TUPLE = list(range(3, 51))
# the families in constraint order, with their sizes; the kinds: every row but the last for step_*, the last for last_row
FAMILIES = [("flags", 2), ("filter", 1), ("first", 16), ("state_bits", 768), ("product_bits", 512), ("carry_bits", 640),
            ("limbs", 48), ("multiply", 16), ("square", 16), ("out", 16), ("step_p", 16), ("step_r", 16), ("step_e", 256),
            ("step_res", 16), ("end_e", 1), ("end_res", 16), ("last_row", 1)]
N_CONSTRAINTS = sum(c for _, c in FAMILIES)   # 2357
TRANSITIONS = ("step_p", "step_r", "step_e", "step_res")
FIRST_INDEX = {}
for _name, _count in FAMILIES:
    FIRST_INDEX[_name] = sum(c for n, c in FAMILIES[:len(FIRST_INDEX)])


def family_of(index):
    """(number, name) of the family constraint `index` belongs to"""
    for k, (name, count) in enumerate(FAMILIES):
        if index < count:
            return k, name
        index -= count
    raise IndexError(index)


def limbs(v):
    return [(v >> (16 * k)) & 0xFFFF for k in range(16)]


def word(ls):
    return sum(l << (16 * k) for k, l in enumerate(ls))


def rows_of(e):
    return max(1, e.bit_length())


# ---------------------------------------------------------------------------------------------- rows and traces
def carries(x, y, product_limbs):
    """the sixteen carries of the truncated schoolbook product: column k + carry in = limb k + 2^16 carry out"""
    out, c = [], 0
    for k in range(16):
        total = sum(x[i] * y[k - i] for i in range(k + 1)) + c
        assert total < 1 << 37
        c = (total - product_limbs[k]) >> 16
        out.append(c)
    return out


def row_of(p, r, e, res, first, last, g, m=None, s=None, out=None):
    """the 2003 cells of a row in state (p, r, e) with final result res: m, s, out as the statement has them unless a
    forgery states them; the carries are what the limb columns and the stated product give"""
    m = (r * p) & M256 if m is None else m
    s = (p * p) & M256 if s is None else s
    out = (m if e & 1 else r) if out is None else out
    row = [0] * N_COLS
    row[G], row[FIRST], row[LAST] = g, first, last
    for col, v in ((P_, p), (E, e), (RES, res), (R, r), (OUT, out)):
        row[col:col + 16] = limbs(v)
    for col, v in ((P_BITS, p), (R_BITS, r), (E_BITS, e), (M_BITS, m), (S_BITS, s)):
        row[col:col + 256] = [(v >> j) & 1 for j in range(256)]
    for col, cs in ((M_CARRY, carries(limbs(r), limbs(p), limbs(m))), (S_CARRY, carries(limbs(p), limbs(p), limbs(s)))):
        for k, c in enumerate(cs):
            row[col + 20 * k:col + 20 * k + 20] = [(c >> j) & 1 for j in range(20)]
    return row


PADDING_ROW = row_of(0, 0, 0, 0, 0, 1, 0)
assert [c for c, v in enumerate(PADDING_ROW) if v] == [LAST]


def chain_rows(base, e, exposed, r=1, n_rows=None, res=None):
    """the rows of one operation: binary exponentiation from the least significant bit.  r, n_rows and res let a forgery
    start from another r, stop early (the last row it writes is flagged last all the same) or state another result."""
    n_rows = rows_of(e) if n_rows is None else n_rows
    states, p = [], base
    for t in range(n_rows):
        states.append((p, r, e))
        if e & 1:
            r = (r * p) & M256
        p, e = (p * p) & M256, e >> 1
    res = r if res is None else res   # r after the last row's step is that row's out
    return [row_of(p, r, e, res, int(t == 0), int(t == n_rows - 1), int(bool(exposed) and t == 0))
            for t, (p, r, e) in enumerate(states)]


def rows_of_ops(ops):
    """the rows of a list of (op, base, exponent, exposed); an op byte other than 1 makes its rows padding rows"""
    rows = []
    for op, base, e, exposed in ops:
        rows += chain_rows(base, e, exposed) if op == EXP else [list(PADDING_ROW) for _ in range(rows_of(e))]
    return rows


def to_trace(rows):
    return np.array([[v % P for v in row] for row in rows], dtype=np.uint64).T.copy()


def trace_of(ops, log_n):
    """[2003, 2^log_n] uint64: the chains one after the other, padding rows to the end"""
    rows = rows_of_ops(ops)
    assert len(rows) <= 1 << log_n
    return to_trace(rows + [list(PADDING_ROW) for _ in range((1 << log_n) - len(rows))])


def first_rows(ops):
    """the row each operation starts at: the exclusive prefix sum of rows_of"""
    out, at = [], 0
    for _, _, e, _ in ops:
        out.append(at)
        at += rows_of(e)
    return out


def tuple_of(base, e, res):
    """the port's tuple for a claim res = base^e"""
    return limbs(base) + limbs(e) + limbs(res)


# ---------------------------------------------------------------------------------------------- the constraints, restated
def constraints(c, n):
    """every constraint at a row with cells c and next row's cells n, as integers mod p, by literal column numbers; the
    kinds are applied by violations()"""
    out = []
    g, first, last, bit = c[0], c[1], c[2], c[595]
    keep = 1 - last

    def value(col, width):
        return sum(c[col + j] << j for j in range(width))

    out += [first * first - first, last * last - last]                               # flags
    out += [g * (1 - first)]                                                         # filter
    out += [first * (c[51 + k] - (k == 0)) for k in range(16)]                       # first
    out += [c[col] * c[col] - c[col] for col in range(83, 851)]                      # state_bits: p, r, e
    out += [c[col] * c[col] - c[col] for col in range(851, 1363)]                    # product_bits: m, s
    out += [c[col] * c[col] - c[col] for col in range(1363, 2003)]                   # carry_bits
    out += [c[3 + k] - value(83 + 16 * k, 16) for k in range(16)]                    # limbs: p
    out += [c[51 + k] - value(339 + 16 * k, 16) for k in range(16)]                  # ... r
    out += [c[19 + k] - value(595 + 16 * k, 16) for k in range(16)]                  # ... e
    m = [value(851 + 16 * k, 16) for k in range(16)]
    s = [value(1107 + 16 * k, 16) for k in range(16)]
    cm = [0] + [value(1363 + 20 * k, 20) for k in range(16)]
    cs = [0] + [value(1683 + 20 * k, 20) for k in range(16)]
    out += [sum(c[51 + i] * c[3 + k - i] for i in range(k + 1)) + cm[k] - m[k] - B * cm[k + 1] for k in range(16)]   # multiply
    out += [sum(c[3 + i] * c[3 + k - i] for i in range(k + 1)) + cs[k] - s[k] - B * cs[k + 1] for k in range(16)]    # square
    out += [c[67 + k] - c[51 + k] - bit * (m[k] - c[51 + k]) for k in range(16)]     # out
    out += [keep * (n[3 + k] - s[k]) for k in range(16)]                             # step_p
    out += [keep * (n[51 + k] - c[67 + k]) for k in range(16)]                       # step_r
    out += [keep * (n[595 + j] - (c[596 + j] if j < 255 else 0)) for j in range(256)]    # step_e
    out += [keep * (n[35 + k] - c[35 + k]) for k in range(16)]                       # step_res
    out += [last * sum(c[596:851])]                                                  # end_e
    out += [last * (c[35 + k] - c[67 + k]) for k in range(16)]                       # end_res
    out += [last - 1]                                                                # last_row
    assert len(out) == N_CONSTRAINTS
    return [v % P for v in out]


def applies(name, row, n_rows):
    """whether family `name` is checked at `row`: a transition everywhere but on the last row, last_row only there"""
    if name in TRANSITIONS:
        return row != n_rows - 1
    return name != "last_row" or row == n_rows - 1


def violations(trace, rows=None):
    """[(row, family, constraint index)] over the whole trace (or `rows`), the next row of the last one being row 0"""
    n = trace.shape[1]
    out = []
    for i in (range(n) if rows is None else rows):
        c, nx = [int(v) for v in trace[:, i]], [int(v) for v in trace[:, (i + 1) % n]]
        for k, v in enumerate(constraints(c, nx)):
            name = family_of(k)[1]
            if v and applies(name, i, n):
                out.append((i, name, k))
    return out


# ---------------------------------------------------------------------------------------------- the edge lists
ONES = M256                      # all-0xFFFF limbs
SIXTY_FOUR = (1 << 64) + 1
LARGEST_CARRY = 0xFFFEF          # out of column 15 of ONES * ONES: AIR 7's figure, which needs all 20 bits


def random_ops(n_rows, seed):
    """seeded operations with exponents of 0 .. 12 bits, a padding operation now and then, `n_rows` rows in all"""
    rng = random.Random(seed)
    ops, left = [], n_rows
    while left:
        e = rng.getrandbits(rng.randint(0, min(12, left)))
        if rows_of(e) > left:
            continue
        ops.append((rng.choice((EXP, EXP, EXP, NONE, 7)), rng.getrandbits(rng.choice((8, 64, 200, 256))), e, rng.randint(0, 1)))
        left -= rows_of(e)
    return ops


def edge_ops():
    """2^9 rows, every one used: the edges of the statement, a full 256-row operation, an unexposed operation, a padding
    operation whose words are junk, random operations, and an operation that ends exactly on the trace's last row"""
    ops = [(EXP, 0, 0, 1), (EXP, 0, 1, 1), (EXP, 1, M256, 1), (EXP, M256, 2, 1), (EXP, 2, 255, 1), (EXP, 2, 256, 1),
           (EXP, 3, SIXTY_FOUR, 1), (EXP, ONES, 3, 1), (EXP, 0xABCDEF << 100 | 0x1235, 0x1B35, 0), (NONE, M256, 0x15, 1),
           (0xFF, 7, 0, 1)]
    used = sum(rows_of(o[2]) for o in ops)
    ops += random_ops(512 - used - 9, 0xE8B0)
    return ops + [(EXP, 0x10001, 0x1A5, 1)]   # nine rows, the last of them row 511


def edge_ops_tail():
    """2^9 rows: (2^256 - 1)^(2^256 - 1) -- every row multiplies --, then 256 padding rows"""
    return [(EXP, M256, M256, 1)]


def small_ops():
    """2^5 rows: what the forgeries and the table sets work on.  Operations start at rows 0, 3, 4, 10 (padding), 12, 14,
    16, 17; rows 28 .. 31 are padding."""
    return [(EXP, 3, 5, 1), (EXP, 0, 0, 1), (EXP, 2, 0b101101, 0), (NONE, 7, 3, 1), (EXP, M256, 2, 1), (EXP, ONES, 3, 1),
            (EXP, 0, 1, 0), (EXP, 0xC0FFEE << 200 | 0x12345678 << 60 | 0xBEEF, 0b10110100111, 1)]


SMALL_STARTS = [0, 3, 4, 10, 12, 14, 16, 17]
FREE_ROW = 29                    # a padding row of small_ops() with padding on both sides


def small_ops_to_the_end():
    """2^5 rows, every one used: the last operation ends on row 31"""
    return small_ops()[:-1] + [(EXP, 0xC0FFEE << 200 | 0xBEEF, 0b110110100111011, 1)]


# ---------------------------------------------------------------------------------------------- wrong witnesses
# A forgery rewrites rows of the model trace of small_ops(), given as a list of rows; what it leaves alone stays honest,
# and what it rewrites stays consistent wherever it can.
def _put(rows, at, new):
    rows[at:at + len(new)] = new


def _cut_short(rows):
    """(2, 0b101101) stopped after two rows with res = that row's out: the exponent 0b10110 is still there"""
    _put(rows, 4, chain_rows(2, 0b101101, 0, n_rows=2))


def _off_the_end(rows):
    """a five-row operation started on row 28: row 31 is not last, and res is whatever the prover likes"""
    new = chain_rows(2, 0b11111, 1, res=12345)[:4]
    _put(rows, 28, new)


def _r_not_one(rows):
    """3^5 started from r = 2: every step is right and res = 2 * 243"""
    _put(rows, 0, chain_rows(3, 5, 1, r=2))


def _p_not_the_square(rows):
    """row 1 of 3^5 holds p = 10 for 9 and the chain goes on from there: res = 3 * 100"""
    new = chain_rows(10, 2, 0, r=3)
    res = word(new[-1][RES:RES + 16])
    assert res == 300
    _put(rows, 0, [row_of(3, 1, 5, res, 1, 0, 1)] + [row[:FIRST] + [0] + row[FIRST + 1:] for row in new])


def _multiply_skipped(rows):
    """row 0 of 3^5 states out = r on a 1 bit, and the chain goes on from r = 1: res = 81"""
    new = chain_rows(9, 2, 0, r=1)
    res = word(new[-1][RES:RES + 16])
    assert res == 81
    _put(rows, 0, [row_of(3, 1, 5, res, 1, 0, 1, out=1)] + [row[:FIRST] + [0] + row[FIRST + 1:] for row in new])


def _result_not_handed_on(rows):
    """row 0 of 3^5 is right, out = 3; row 1 starts from r = 1 all the same: res = 81"""
    new = chain_rows(9, 2, 0, r=1)
    _put(rows, 0, [row_of(3, 1, 5, 81, 1, 0, 1)] + [row[:FIRST] + [0] + row[FIRST + 1:] for row in new])


def _bit_dropped(rows):
    """3^5 with the exponent 0 on row 1 for 0b10: that row is the last, res = 3; row 2 is left as it was, a lone row"""
    _put(rows, 0, [row_of(3, 1, 5, 3, 1, 0, 1), row_of(9, 3, 0, 3, 0, 1, 0)])


def _res_changed(rows):
    """(2, 0b101101): rows 4 .. 6 state res + 1, rows 7 .. 9 the result"""
    for i in (4, 5, 6):
        assert rows[i][RES] < 0xFFFF
        rows[i][RES] += 1


def _res_not_out(rows):
    """3^5 = 244, on every row"""
    _put(rows, 0, chain_rows(3, 5, 1, res=244))


def _m_not_the_product(rows):
    """row 0 of 3^5: m = 4 for 3, out and the rest of the chain following it: res = 4 * 81"""
    new = chain_rows(9, 2, 0, r=4)
    _put(rows, 0, [row_of(3, 1, 5, 324, 1, 0, 1, m=4)] + [row[:FIRST] + [0] + row[FIRST + 1:] for row in new])
    rows[0][M_CARRY:M_CARRY + 320] = [0] * 320   # 3 - 4 < 0: the carries the honest product has


def _s_not_the_square(rows):
    """row 0 of 3^5: s = 10 for 9, p' following it"""
    _p_not_the_square(rows)
    rows[0][S_BITS:S_BITS + 256] = [(10 >> j) & 1 for j in range(256)]
    rows[0][S_CARRY:S_CARRY + 320] = [0] * 320


def _carry_out_of_range(rows):
    """the last carry of r p on row 14 ((2^256 - 1)^3), the one that is discarded, with 2^20 more: bit 19 holds 2 more"""
    rows[14][M_CARRY + 20 * 15 + 19] += 2


def _fat_limb(rows):
    """row 17: the limb column e_0 holds e_0 + 2^16; its bits cannot"""
    rows[17][E] += B


def _non_bit(col, row):
    def forge(rows):
        """bits (0, 1) of a block's value written as (2, 0): the same value"""
        j = next(j for j in range(1, 15) if (rows[row][col + j], rows[row][col + j + 1]) == (0, 1))
        rows[row][col + j], rows[row][col + j + 1] = 2, 0
    return forge


def _g_not_first(rows):
    rows[1][G] = 1


def _exposed_padding(rows):
    rows[FREE_ROW][G] = 1


def _flag_no_bit(rows):
    """last = 2 on a padding row between padding rows: keep = -1 switches nothing on there"""
    rows[FREE_ROW][LAST] = 2


# (name, the forgery, the (row, family) pairs that break -- nothing else may)
CATALOGUE = [("chain_cut_short", _cut_short, {(5, "end_e")}),
             ("chain_off_the_traces_end", _off_the_end, {(31, "last_row")}),
             ("r_not_one_on_a_first_row", _r_not_one, {(0, "first")}),
             ("next_p_not_the_square", _p_not_the_square, {(0, "step_p")}),
             ("multiply_skipped_on_a_one_bit", _multiply_skipped, {(0, "out")}),
             ("result_not_handed_on", _result_not_handed_on, {(0, "step_r")}),
             ("exponent_bit_dropped_in_the_shift", _bit_dropped, {(0, "step_e")}),
             ("res_changed_in_mid_chain", _res_changed, {(6, "step_res")}),
             ("res_not_out_on_the_last_row", _res_not_out, {(2, "end_res")}),
             ("m_not_the_product", _m_not_the_product, {(0, "multiply")}),
             ("s_not_the_square", _s_not_the_square, {(0, "square")}),
             ("carry_out_of_range", _carry_out_of_range, {(14, "carry_bits"), (14, "multiply")}),
             ("limb_of_two_to_the_16", _fat_limb, {(17, "limbs")}),
             ("non_bit_in_p", _non_bit(P_BITS, 19), {(19, "state_bits")}),
             ("non_bit_in_r", _non_bit(R_BITS, 20), {(20, "state_bits")}),
             ("non_bit_in_e", _non_bit(E_BITS, 4), {(4, "state_bits"), (4, "step_e")}),
             ("non_bit_in_m", _non_bit(M_BITS, 19), {(19, "product_bits")}),
             ("non_bit_in_s", _non_bit(S_BITS, 19), {(19, "product_bits")}),
             ("non_bit_in_a_carry_of_r_p", _non_bit(M_CARRY + 20 * 7, 20), {(20, "carry_bits")}),
             ("non_bit_in_a_carry_of_p_p", _non_bit(S_CARRY + 20 * 7, 14), {(14, "carry_bits")}),
             ("g_on_a_row_that_is_not_first", _g_not_first, {(1, "filter")}),
             ("exposed_padding_row", _exposed_padding, {(FREE_ROW, "filter")}),
             ("flag_that_is_no_bit", _flag_no_bit, {(FREE_ROW, "flags")})]


def forged(entry):
    """the model trace of small_ops() with a catalogue entry's forgery applied: [2003, 32] uint64"""
    rows = rows_of_ops(small_ops())
    rows += [list(PADDING_ROW) for _ in range(32 - len(rows))]
    entry[1](rows)
    assert len(rows) == 32
    return to_trace(rows)
