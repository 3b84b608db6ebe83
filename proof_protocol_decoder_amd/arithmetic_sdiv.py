"""The signed table: SDIV and SMOD on 256-bit words, one operation per row -- the fourth constraint program shipped with
the package (air_program.Builder, registered at run time: no built-in air_id) and the witness generator behind
bp_arithmetic_sdiv_trace (csrc/arithmetic_sdiv.hip).  AIRS.md section 2, "Signed (a shipped program)", states the layout
and the soundness notes; include/bpg.h the statement and the input words.

    air_id = arithmetic_sdiv.register()                      # once per process; raises if the kernel's column map differs
    trace = ops.arithmetic_sdiv_trace(log_n, to_device(arithmetic_sdiv.pack_inputs([(SDIV, x, y, 1), (SMOD, x, y, 0)])))
    op, x, y, q, r, res, g = arithmetic_sdiv.unpack_row(trace_on_host, 0)

With sx, sy the bits 255 of x and y and X = x - sx 2^256, Y = y - sy 2^256: every row proves ax = |X|, ay = |Y| (a
conditional negation chain each), q ay + r = ax over the integers and r < ay unless y = 0 (the division table's core, on
the magnitudes), and res = m or -m mod 2^256 (a third chain) for the magnitude m = 0 (y = 0), q (is_sdiv), r (is_smod)
and the sign neg = sx xor sy (is_sdiv), sx (is_smod): the quotient rounds toward zero, the remainder has the sign of x.
The one product port exposes (is_sdiv, is_smod, x limbs, y limbs, res limbs) on the rows whose filter column g is 1.
"""
from . import word_table
from .air_program import ALL_ROWS, Builder
from .word_table import BASE, LIMB_BITS, _word, bits_sum, bits_value, negation_limb, remainder_limb

OP_NONE, OP_SDIV, OP_SMOD = 0, 1, 2
LIMBS, CARRY_BITS, N_CARRIES = 16, 19, 15
WORD_BITS = LIMBS * LIMB_BITS

# ---- the column map (bp_arithmetic_sdiv_layout states the kernel's)
COL_IS_SDIV, COL_IS_SMOD, COL_G, COL_Z, COL_INV, COL_NEG = 0, 1, 2, 3, 4, 5
COL_X = 6                               # sixteen 16-bit limbs of x, least significant first
COL_Y = COL_X + LIMBS                   # ... of y
COL_RES = COL_Y + LIMBS                 # ... of the result
COL_Q = COL_RES + LIMBS                 # ... of the quotient of the magnitudes
COL_AY = COL_Q + LIMBS                  # ... of ay = |Y|
COL_M = COL_AY + LIMBS                  # ... of the result's magnitude m
COL_X_BITS = COL_M + LIMBS              # bit j of limb k at + 16 k + j, for x, y, res, ax = |X|, ay, q, r and the slack d = ay - r - 1
COL_Y_BITS = COL_X_BITS + WORD_BITS
COL_RES_BITS = COL_Y_BITS + WORD_BITS
COL_AX_BITS = COL_RES_BITS + WORD_BITS
COL_AY_BITS = COL_AX_BITS + WORD_BITS
COL_Q_BITS = COL_AY_BITS + WORD_BITS
COL_R_BITS = COL_Q_BITS + WORD_BITS
COL_D_BITS = COL_R_BITS + WORD_BITS
COL_CARRY = COL_D_BITS + WORD_BITS      # bit j of the carry out of product column k (k < 15) at + 19 k + j
COL_BORROW = COL_CARRY + N_CARRIES * CARRY_BITS   # the carry bit out of limb k of r + d + 1
COL_X_CHAIN = COL_BORROW + LIMBS        # the carry bit out of limb k of x + ax, of y + ay, of m + res
COL_Y_CHAIN = COL_X_CHAIN + LIMBS
COL_RES_CHAIN = COL_Y_CHAIN + LIMBS
N_COLS = COL_RES_CHAIN + LIMBS          # 2499
LAYOUT = (N_COLS, COL_IS_SDIV, COL_IS_SMOD, COL_G, COL_Z, COL_INV, COL_NEG, COL_X, COL_Y, COL_RES, COL_Q, COL_AY, COL_M,
          COL_X_BITS, COL_Y_BITS, COL_RES_BITS, COL_AX_BITS, COL_AY_BITS, COL_Q_BITS, COL_R_BITS, COL_D_BITS, COL_CARRY,
          CARRY_BITS, COL_BORROW, COL_X_CHAIN, COL_Y_CHAIN, COL_RES_CHAIN)
TUPLE_COLS = (COL_IS_SDIV, COL_IS_SMOD) + tuple(range(COL_X, COL_X + 3 * LIMBS))   # the port's 50 elements

# ---- the constraint list: (name, count, degree), all of kind ALL_ROWS, in index order
FAMILIES = (("flags", 3, 2),            # is_sdiv, is_smod, z are bits
            ("one_flag", 1, 2),         # is_sdiv is_smod
            ("filter", 1, 2),           # g (1 - is_sdiv - is_smod)
            ("zero", 2, 2),             # z S, S inv - (1 - z) with S = sum of y's limbs
            ("high", 1, 2),             # sum_{i + j >= 16} q_i ay_j
            ("neg", 1, 3),              # neg - is_sdiv (sx + sy - 2 sx sy) - is_smod sx
            ("operand_bits", 3 * WORD_BITS, 2),     # the bits of x, then of y, then of res
            ("magnitude_bits", 2 * WORD_BITS, 2),   # the bits of ax, then of ay
            ("core_bits", 3 * WORD_BITS, 2),        # the bits of q, then of r, then of d
            ("carry_bits", N_CARRIES * CARRY_BITS, 2), ("borrow_bits", LIMBS, 2),
            ("chain_bits", 3 * LIMBS, 2),           # the carry bits of x + ax, then of y + ay, then of m + res
            ("limbs", 5 * LIMBS, 1),    # limb column - sum of its bits: x_k at k, y_k at 16 + k, then res_k, q_k, ay_k
            ("magnitude", 2 * LIMBS, 2),   # (ax_k - x_k) + sx (2 x_k + c_{k-1} - 2^16 c_k) at k; the same for y, ay, sy at 16 + k
            ("product", LIMBS, 2),      # sum_{i + j = k} q_i ay_j + r_k + c_{k-1} - ax_k - 2^16 c_k  (no c_15)
            ("remainder", LIMBS, 2),    # (1 - z) (r_k + d_k + [k = 0] + b_{k-1} - ay_k - 2^16 b_k)
            ("remainder_top", 1, 2),    # (1 - z) b_15
            ("m", LIMBS, 3),            # m_k - (1 - z) (is_sdiv q_k + is_smod r_k)
            ("result", LIMBS, 2))       # (res_k - m_k) + neg (2 m_k + c_{k-1} - 2^16 c_k)
FAMILY_INDEX = {name: k for k, (name, _, _) in enumerate(FAMILIES)}
# Limbs a unit after the first unit.  At 2^14 rows on an MI355X one limb a unit (18 units with the port's: 9 workgroup
# rows of two) is 1,016 us in K5 and 13.49 ms a proof, two (10 rows of one) 1,008 us and 13.46 ms, the ranges overlapping
# (profiles/arithmetic_sdiv.txt): the timings pick neither, and one needs 9 registers where two needs 11.
CUTS = (1, 2)
LIMBS_PER_UNIT = 1


def first_index(name):
    """the constraint index at which family `name` starts"""
    return word_table.first_index(FAMILIES, name)


def program(limbs_per_unit=LIMBS_PER_UNIT):
    """The table's air_program.Builder: the unit of the flags, the zero test, the sign and the high half of q ay; then
    one unit per `limbs_per_unit` limbs, which sums the bits of those limbs once; and the looked port."""
    if limbs_per_unit not in CUTS:
        raise ValueError("limbs_per_unit is one of %s" % (CUTS,))
    b = Builder(N_COLS)
    at = {name: b.family(count, ALL_ROWS, degree) for name, count, degree in FAMILIES}
    is_sdiv, is_smod, g, z = b.loc(COL_IS_SDIV), b.loc(COL_IS_SMOD), b.loc(COL_G), b.loc(COL_Z)
    neg, sx, sy = b.loc(COL_NEG), b.loc(COL_X_BITS + WORD_BITS - 1), b.loc(COL_Y_BITS + WORD_BITS - 1)
    not_zero = 1 - z

    b.unit()
    word_table.flags(b, at, is_sdiv, is_smod, g, z)
    b.emit(at["neg"], neg - (is_sdiv * ((sx + sy) - 2 * (sx * sy)) + is_smod * sx))
    # T_i = ay_15 + ... + ay_(16 - i): q_i T_i sums the products of q_i that land in columns 16 .. 30
    suffix, high, s = 0, 0, 0
    for i in range(1, LIMBS):
        suffix = suffix + b.loc(COL_AY + LIMBS - i)
        high = high + b.loc(COL_Q + i) * suffix
    b.emit(at["high"], high)
    for j in range(LIMBS):
        s = s + b.loc(COL_Y + j)
    word_table.zero_test(b, at, z, s, b.loc(COL_INV), not_zero)

    def block(j, col, family, k):   # limb k of word j of a family of bit blocks
        return bits_value(b, col + LIMB_BITS * k, LIMB_BITS, at[family] + WORD_BITS * j + LIMB_BITS * k)

    carry = borrow = 0
    for k in range(LIMBS):
        if k % limbs_per_unit == 0:
            b.unit()
            if k:   # the carries into this unit's first limb, summed again here: registers do not live across units
                carry = bits_sum(b, COL_CARRY + CARRY_BITS * (k - 1), CARRY_BITS)
                borrow = b.loc(COL_BORROW + k - 1)
        xk, yk, resk = block(0, COL_X_BITS, "operand_bits", k), block(1, COL_Y_BITS, "operand_bits", k), block(2, COL_RES_BITS, "operand_bits", k)
        axk, ayk = block(0, COL_AX_BITS, "magnitude_bits", k), block(1, COL_AY_BITS, "magnitude_bits", k)
        qk, rk, dk = block(0, COL_Q_BITS, "core_bits", k), block(1, COL_R_BITS, "core_bits", k), block(2, COL_D_BITS, "core_bits", k)
        for j, (col, value) in enumerate(((COL_X, xk), (COL_Y, yk), (COL_RES, resk), (COL_Q, qk), (COL_AY, ayk))):
            b.emit(at["limbs"] + LIMBS * j + k, b.loc(col + k) - value)
        negation_limb(b, k, sx, xk, axk, COL_X_CHAIN, at["chain_bits"], at["magnitude"])
        negation_limb(b, k, sy, yk, ayk, COL_Y_CHAIN, at["chain_bits"] + LIMBS, at["magnitude"] + LIMBS)
        conv = 0
        for i in range(k + 1):
            conv = conv + b.loc(COL_Q + i) * b.loc(COL_AY + k - i)
        if k < N_CARRIES:
            out = bits_value(b, COL_CARRY + CARRY_BITS * k, CARRY_BITS, at["carry_bits"] + CARRY_BITS * k)
            b.emit(at["product"] + k, (conv + rk + carry) - (axk + BASE * out))
            carry = out
        else:
            b.emit(at["product"] + k, (conv + rk + carry) - axk)
        borrow = remainder_limb(b, at, k, rk, dk, ayk, borrow, COL_BORROW, not_zero)
        mk = b.loc(COL_M + k)
        b.emit(at["m"] + k, mk - not_zero * (is_sdiv * b.loc(COL_Q + k) + is_smod * rk))
        negation_limb(b, k, neg, mk, resk, COL_RES_CHAIN, at["chain_bits"] + 2 * LIMBS, at["result"])
    b.emit(at["remainder_top"], not_zero * borrow)
    b.port(g, [b.loc(c) for c in TUPLE_COLS])
    return b


def kernel_layout():
    """bp_arithmetic_sdiv_layout: the column map csrc/arithmetic_sdiv.hip stores by, in LAYOUT's order"""
    return word_table.kernel_layout("bp_arithmetic_sdiv_layout", len(LAYOUT))


def register():
    """Assembles and registers the program (once per process) and returns its air_id.  The column map exists twice, here
    and in the witness kernel: RuntimeError if the two disagree."""
    return word_table.register("arithmetic_sdiv", LAYOUT, "bp_arithmetic_sdiv_layout", program)


def pack_inputs(ops_list):
    """[(op, x, y, exposed), ...] of Python integers -> the [n, 9] uint64 input words of bp_arithmetic_sdiv_trace: word 0
    = op (1 sdiv, 2 smod, else a padding row) | exposed << 8, then the four 64-bit words of x and of y, two's complement,
    least significant first: the division table's format"""
    return word_table.pack_inputs(ops_list, 2, "x and y")


def unpack_row(trace, i):
    """(op, x, y, q, r, res, g) of row i of a [N_COLS, n] trace (anything indexable as trace[col][row]) as Python
    integers: the words x, y, res and the quotient of the magnitudes from their limb columns, the magnitudes' remainder
    from its bits"""
    cells = [int(trace[c][i]) for c in range(COL_D_BITS)]
    op = OP_SDIV if cells[COL_IS_SDIV] else OP_SMOD if cells[COL_IS_SMOD] else OP_NONE
    return (op, _word(cells, COL_X, LIMB_BITS, LIMBS), _word(cells, COL_Y, LIMB_BITS, LIMBS),
            _word(cells, COL_Q, LIMB_BITS, LIMBS), _word(cells, COL_R_BITS, 1, WORD_BITS), _word(cells, COL_RES, LIMB_BITS, LIMBS),
            cells[COL_G])
