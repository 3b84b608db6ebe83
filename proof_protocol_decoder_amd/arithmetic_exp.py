"""The exponentiation table: EXP on 256-bit words, one exponent bit per row -- the fifth constraint program shipped with
the package (air_program.Builder, registered at run time: no built-in air_id), the first whose statement spans rows, and
the witness generator behind bp_arithmetic_exp_trace (csrc/arithmetic_exp.hip).  AIRS.md section 2, "Exponentiation (a
shipped program)", states the layout and the soundness notes; include/bpg.h the statement and the input words.

    air_id = arithmetic_exp.register()                       # once per process; raises if the kernel's column map differs
    words, starts = arithmetic_exp.pack_ops([(EXP, 3, 5, 1), (EXP, 2, 256, 0)], log_n)
    trace = ops.arithmetic_exp_trace(log_n, words_on_device, starts_on_device)
    first, last, base, exponent, res, g = arithmetic_exp.unpack_row(trace_on_host, 0)

An operation is a chain of rows_of(exponent) = max(1, bit length) consecutive rows: binary exponentiation from the least
significant bit.  A row holds the running square p, the running result r, the exponent e still to consume and the final
result res; with bit = e's bit 0, m = r p mod 2^256 and s = p p mod 2^256 it proves both truncated products and out =
bit ? m : r, and unless its flag `last` is set the next row has p' = s, r' = out, e' = e >> 1, res' = res.  A `last` row
has e < 2 and res = out, a `first` row r = 1: r p^e = base^exponent mod 2^256 on the first row, a step keeps it, so res =
base^exponent mod 2^256.  The one product port exposes (p limbs, e limbs, res limbs) -- on a first row (base, exponent,
res) -- on the rows whose filter column g is 1, and g may be 1 on a first row only.
"""
import numpy as np

from . import word_table
from .air_program import ALL_ROWS, LAST_ROW, TRANSITION, Builder
from .word_table import BASE, LIMB_BITS, _word, bits_sum, bits_value

OP_NONE, OP_EXP = 0, 1
LIMBS, CARRY_BITS = 16, 20
WORD_BITS = LIMBS * LIMB_BITS
MAX_ROWS = WORD_BITS                    # the longest chain: an exponent with bit 255 set

# ---- the column map (bp_arithmetic_exp_layout states the kernel's)
COL_G, COL_FIRST, COL_LAST = 0, 1, 2
COL_P = 3                               # sixteen 16-bit limbs of the running square p, least significant first
COL_E = COL_P + LIMBS                   # ... of the exponent still to consume
COL_RES = COL_E + LIMBS                 # ... of the chain's final result
COL_R = COL_RES + LIMBS                 # ... of the running result r
COL_OUT = COL_R + LIMBS                 # ... of out = bit ? m : r
COL_P_BITS = COL_OUT + LIMBS            # bit j of limb k at + 16 k + j, for p, r, e, m = r p and s = p p (mod 2^256)
COL_R_BITS = COL_P_BITS + WORD_BITS
COL_E_BITS = COL_R_BITS + WORD_BITS
COL_M_BITS = COL_E_BITS + WORD_BITS
COL_S_BITS = COL_M_BITS + WORD_BITS
COL_M_CARRY = COL_S_BITS + WORD_BITS    # bit j of the carry out of column k of r p at + 20 k + j, k = 0 .. 15
COL_S_CARRY = COL_M_CARRY + LIMBS * CARRY_BITS   # ... of p p
N_COLS = COL_S_CARRY + LIMBS * CARRY_BITS        # 2003
LAYOUT = (N_COLS, COL_G, COL_FIRST, COL_LAST, COL_P, COL_E, COL_RES, COL_R, COL_OUT, COL_P_BITS, COL_R_BITS, COL_E_BITS,
          COL_M_BITS, COL_S_BITS, COL_M_CARRY, COL_S_CARRY, CARRY_BITS)
TUPLE_COLS = tuple(range(COL_P, COL_P + 3 * LIMBS))   # the port's 48 elements

# ---- the constraint list: (name, count, kind, degree), in index order.  keep = 1 - last.
FAMILIES = (("flags", 2, ALL_ROWS, 2),          # first, last are bits
            ("filter", 1, ALL_ROWS, 2),         # g (1 - first)
            ("first", LIMBS, ALL_ROWS, 2),      # first (r_k - [k = 0])
            ("state_bits", 3 * WORD_BITS, ALL_ROWS, 2),     # the bits of p, then of r, then of e
            ("product_bits", 2 * WORD_BITS, ALL_ROWS, 2),   # the bits of m, then of s
            ("carry_bits", 2 * LIMBS * CARRY_BITS, ALL_ROWS, 2),   # the carries of r p, then of p p
            ("limbs", 3 * LIMBS, ALL_ROWS, 1),  # limb column - sum of its bits: p_k at k, r_k at 16 + k, e_k at 32 + k
            ("multiply", LIMBS, ALL_ROWS, 2),   # sum_{i + j = k} r_i p_j + c_(k-1) - m_k - 2^16 c_k
            ("square", LIMBS, ALL_ROWS, 2),     # sum_{i + j = k} p_i p_j + c_(k-1) - s_k - 2^16 c_k
            ("out", LIMBS, ALL_ROWS, 2),        # out_k - r_k - bit (m_k - r_k)
            ("step_p", LIMBS, TRANSITION, 2),   # keep (p'_k - s_k)
            ("step_r", LIMBS, TRANSITION, 2),   # keep (r'_k - out_k)
            ("step_e", WORD_BITS, TRANSITION, 2),   # keep (e'_j - e_(j+1)), keep e'_255
            ("step_res", LIMBS, TRANSITION, 2),     # keep (res'_k - res_k)
            ("end_e", 1, ALL_ROWS, 2),          # last (e_1 + ... + e_255)
            ("end_res", LIMBS, ALL_ROWS, 2),    # last (res_k - out_k)
            ("last_row", 1, LAST_ROW, 1))       # last - 1 on the trace's last row
FAMILY_INDEX = {name: k for k, (name, _, _, _) in enumerate(FAMILIES)}
# Limbs a unit after the first unit.  At 2^14 rows on an MI355X one limb a unit (18 units with the port's: 9 workgroup
# rows of two) is 1,050 us in K5 and 11.79 ms a proof, two (10 rows of one) 1,074 us and 11.82 ms, four (6 rows) 1,493 us
# and 12.30 ms (profiles/arithmetic_exp.txt): one is the fastest in K5 and needs 7 registers where two and four need 8 and 9.
CUTS = (1, 2, 4)
LIMBS_PER_UNIT = 1


def rows_of(exponent):
    """the rows an operation takes: one per exponent bit up to the highest set, one for an exponent of zero"""
    return max(1, int(exponent).bit_length())


def first_index(name):
    """the constraint index at which family `name` starts"""
    return word_table.first_index(FAMILIES, name)


def program(limbs_per_unit=LIMBS_PER_UNIT):
    """The table's air_program.Builder: the unit of the flags, the end of the exponent and the boundary; then one unit
    per `limbs_per_unit` limbs, which sums the bits of those limbs once; and the looked port."""
    if limbs_per_unit not in CUTS:
        raise ValueError("limbs_per_unit is one of %s" % (CUTS,))
    b = Builder(N_COLS)
    at = {name: b.family(count, kind, degree) for name, count, kind, degree in FAMILIES}
    g, first, last, bit = b.loc(COL_G), b.loc(COL_FIRST), b.loc(COL_LAST), b.loc(COL_E_BITS)
    keep = 1 - last

    b.unit()
    b.emit(at["flags"], first * first - first)
    b.emit(at["flags"] + 1, last * last - last)
    b.emit(at["filter"], g * (1 - first))
    rest = 0
    for j in range(1, WORD_BITS):   # a sum of bits: zero only if every one is
        rest = rest + b.loc(COL_E_BITS + j)
    b.emit(at["end_e"], last * rest)
    b.emit(at["last_row"], last - 1)

    def block(j, col, family, k):   # limb k of word j of a family of bit blocks
        return bits_value(b, col + LIMB_BITS * k, LIMB_BITS, at[family] + WORD_BITS * j + LIMB_BITS * k)

    carry_m = carry_s = 0
    for k in range(LIMBS):
        if k % limbs_per_unit == 0:
            b.unit()
            if k:   # the carries into this unit's first limb, summed again here: registers do not live across units
                carry_m = bits_sum(b, COL_M_CARRY + CARRY_BITS * (k - 1), CARRY_BITS)
                carry_s = bits_sum(b, COL_S_CARRY + CARRY_BITS * (k - 1), CARRY_BITS)
        pk, rk, ek = block(0, COL_P_BITS, "state_bits", k), block(1, COL_R_BITS, "state_bits", k), block(2, COL_E_BITS, "state_bits", k)
        mk, sk = block(0, COL_M_BITS, "product_bits", k), block(1, COL_S_BITS, "product_bits", k)
        for j, (col, value) in enumerate(((COL_P, pk), (COL_R, rk), (COL_E, ek))):
            b.emit(at["limbs"] + LIMBS * j + k, b.loc(col + k) - value)
        conv_m = conv_s = 0
        for i in range(k + 1):
            conv_m = conv_m + b.loc(COL_R + i) * b.loc(COL_P + k - i)
        for i in range((k + 1) // 2):   # p_i p_(k-i) twice, the middle one once
            conv_s = conv_s + b.loc(COL_P + i) * b.loc(COL_P + k - i)
        conv_s = conv_s + conv_s
        if k % 2 == 0:
            conv_s = conv_s + b.loc(COL_P + k // 2) * b.loc(COL_P + k // 2)
        out_m = bits_value(b, COL_M_CARRY + CARRY_BITS * k, CARRY_BITS, at["carry_bits"] + CARRY_BITS * k)
        b.emit(at["multiply"] + k, (conv_m + carry_m) - (mk + BASE * out_m))
        out_s = bits_value(b, COL_S_CARRY + CARRY_BITS * k, CARRY_BITS, at["carry_bits"] + CARRY_BITS * (LIMBS + k))
        b.emit(at["square"] + k, (conv_s + carry_s) - (sk + BASE * out_s))
        carry_m, carry_s = out_m, out_s
        outk = b.loc(COL_OUT + k)
        b.emit(at["out"] + k, (outk - rk) - bit * (mk - rk))
        b.emit(at["first"] + k, first * (rk - (1 if k == 0 else 0)))
        b.emit(at["step_p"] + k, keep * (b.nxt(COL_P + k) - sk))
        b.emit(at["step_r"] + k, keep * (b.nxt(COL_R + k) - outk))
        for j in range(LIMB_BITS * k, LIMB_BITS * (k + 1)):
            above = b.loc(COL_E_BITS + j + 1) if j + 1 < WORD_BITS else 0
            b.emit(at["step_e"] + j, keep * (b.nxt(COL_E_BITS + j) - above))
        b.emit(at["step_res"] + k, keep * (b.nxt(COL_RES + k) - b.loc(COL_RES + k)))
        b.emit(at["end_res"] + k, last * (b.loc(COL_RES + k) - outk))
    b.port(g, [b.loc(c) for c in TUPLE_COLS])
    return b


def kernel_layout():
    """bp_arithmetic_exp_layout: the column map csrc/arithmetic_exp.hip stores by, in LAYOUT's order"""
    return word_table.kernel_layout("bp_arithmetic_exp_layout", len(LAYOUT))


def register():
    """Assembles and registers the program (once per process) and returns its air_id.  The column map exists twice, here
    and in the witness kernel: RuntimeError if the two disagree."""
    return word_table.register("arithmetic_exp", LAYOUT, "bp_arithmetic_exp_layout", program)


def pack_ops(ops_list, log_n):
    """[(op, base, exponent, exposed), ...] of Python integers -> (words, starts) for bp_arithmetic_exp_trace: words is
    [n_ops, 9] uint64 (word 0 = op (1 exp, else the operation's rows are padding) | exposed << 8, then the four 64-bit
    words of the base and of the exponent, least significant first), starts [n_ops + 1] uint32, the exclusive prefix sum
    of rows_of(exponent).  ValueError when the operations need more than 2^log_n rows."""
    words = word_table.pack_inputs(ops_list, 2, "base and exponent")
    starts = np.zeros(len(ops_list) + 1, dtype=np.uint32)
    total = 0
    for i, op in enumerate(ops_list):
        total += rows_of(op[2])
        if total > 1 << log_n:
            raise ValueError("operation %d ends at row %d: the trace has 2^%d rows" % (i, total, log_n))
        starts[i + 1] = total
    return words, starts


def unpack_row(trace, i):
    """(first, last, p, e, res, g) of row i of a [N_COLS, n] trace (anything indexable as trace[col][row]) as Python
    integers; on a first row p is the base and e the exponent"""
    cells = [int(trace[c][i]) for c in range(COL_R)]
    return (cells[COL_FIRST], cells[COL_LAST], _word(cells, COL_P, LIMB_BITS, LIMBS), _word(cells, COL_E, LIMB_BITS, LIMBS),
            _word(cells, COL_RES, LIMB_BITS, LIMBS), cells[COL_G])
