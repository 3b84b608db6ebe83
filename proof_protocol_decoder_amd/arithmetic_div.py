"""The division table: DIV and MOD on 256-bit words, one operation per row -- a constraint program shipped with the
package (air_program.Builder, registered at run time: no built-in air_id) and the witness generator behind
bp_arithmetic_div_trace (csrc/arithmetic_div.hip).  AIRS.md section 2, "Division (a shipped program)", states the
layout and the soundness notes; include/bpg.h the statement and the input words.

    air_id = arithmetic_div.register()                       # once per process; raises if the kernel's column map differs
    trace = ops.arithmetic_div_trace(log_n, to_device(arithmetic_div.pack_inputs([(DIV, x, y, 1), (MOD, x, y, 0)])))
    op, x, y, q, r, res, g = arithmetic_div.unpack_row(trace_on_host, 0)

Every row proves q y + r = x over the integers, r < y unless y = 0, and res = 0 (y = 0), q (is_div), r (is_mod).  The
one product port exposes (is_div, is_mod, x limbs, y limbs, res limbs) on the rows whose filter column g is 1.
"""
from . import word_table
from .air_program import ALL_ROWS, Builder
from .word_table import BASE, EXPOSED, LIMB_BITS, _word, bits_sum, bits_value, remainder_limb

OP_NONE, OP_DIV, OP_MOD = 0, 1, 2
LIMBS, CARRY_BITS, N_CARRIES = 16, 19, 15

# ---- the column map (bp_arithmetic_div_layout states the kernel's)
COL_IS_DIV, COL_IS_MOD, COL_G, COL_Z, COL_INV = 0, 1, 2, 3, 4
COL_X = 5                               # sixteen 16-bit limbs of x, least significant first
COL_Y = COL_X + LIMBS                   # ... of y
COL_RES = COL_Y + LIMBS                 # ... of the result
COL_Q = COL_RES + LIMBS                 # ... of the quotient
COL_X_BITS = COL_Q + LIMBS              # bit j of limb k at + 16 k + j, for x, y, q, r and the slack d = y - r - 1
COL_Y_BITS = COL_X_BITS + LIMBS * LIMB_BITS
COL_Q_BITS = COL_Y_BITS + LIMBS * LIMB_BITS
COL_R_BITS = COL_Q_BITS + LIMBS * LIMB_BITS
COL_D_BITS = COL_R_BITS + LIMBS * LIMB_BITS
COL_CARRY = COL_D_BITS + LIMBS * LIMB_BITS   # bit j of the carry out of product column k (k < 15) at + 19 k + j
COL_BORROW = COL_CARRY + N_CARRIES * CARRY_BITS   # the carry bit out of limb k of r + d + 1
N_COLS = COL_BORROW + LIMBS             # 1650
LAYOUT = (N_COLS, COL_IS_DIV, COL_IS_MOD, COL_G, COL_Z, COL_INV, COL_X, COL_Y, COL_RES, COL_Q, COL_X_BITS, COL_Y_BITS,
          COL_Q_BITS, COL_R_BITS, COL_D_BITS, COL_CARRY, CARRY_BITS, COL_BORROW)
TUPLE_COLS = (COL_IS_DIV, COL_IS_MOD) + tuple(range(COL_X, COL_X + 3 * LIMBS))   # the port's 50 elements

# ---- the constraint list: (name, count, degree), all of kind ALL_ROWS, in index order
FAMILIES = (("flags", 3, 2),            # is_div, is_mod, z are bits
            ("one_flag", 1, 2),         # is_div is_mod
            ("filter", 1, 2),           # g (1 - is_div - is_mod)
            ("zero", 2, 2),             # z S, S inv - (1 - z) with S = sum of y's limbs
            ("high", 1, 2),             # sum_{i + j >= 16} q_i y_j
            ("x_bits", 256, 2), ("y_bits", 256, 2), ("q_bits", 256, 2), ("r_bits", 256, 2), ("d_bits", 256, 2),
            ("carry_bits", N_CARRIES * CARRY_BITS, 2), ("borrow_bits", LIMBS, 2),
            ("x_limbs", LIMBS, 1), ("y_limbs", LIMBS, 1), ("q_limbs", LIMBS, 1),   # limb column - sum of its bits
            ("product", LIMBS, 2),      # sum_{i + j = k} q_i y_j + r_k + c_{k-1} - x_k - 2^16 c_k  (no c_15)
            ("remainder", LIMBS, 2),    # (1 - z) (r_k + d_k + [k = 0] + b_{k-1} - y_k - 2^16 b_k)
            ("remainder_top", 1, 2),    # (1 - z) b_15
            ("result", LIMBS, 3))       # res_k - (1 - z) (is_div q_k + is_mod r_k)
FAMILY_INDEX = {name: k for k, (name, _, _) in enumerate(FAMILIES)}
# Two limbs a unit (nine units with the first): at 2^14 rows a proof takes 9.5 ms on an MI355X with one or two limbs a
# unit, 9.95 ms with four, 10.9 with eight, 12.7 with sixteen -- more units fill the chip's grid.y.
LIMBS_PER_UNIT = 2


def first_index(name):
    """the constraint index at which family `name` starts"""
    return word_table.first_index(FAMILIES, name)


def program(limbs_per_unit=LIMBS_PER_UNIT):
    """The table's air_program.Builder: the unit of the flags, the zero test and the high half of q y; then one unit per
    `limbs_per_unit` limbs, which sums the bits of those limbs once; and the looked port."""
    b = Builder(N_COLS)
    at = {name: b.family(count, ALL_ROWS, degree) for name, count, degree in FAMILIES}
    is_div, is_mod, g, z = b.loc(COL_IS_DIV), b.loc(COL_IS_MOD), b.loc(COL_G), b.loc(COL_Z)
    not_zero = 1 - z

    b.unit()
    word_table.flags(b, at, is_div, is_mod, g, z)
    # T_i = y_15 + ... + y_(16 - i): q_i T_i sums the products of q_i that land in columns 16 .. 30; T_16 = S
    suffix, high = 0, 0
    for i in range(1, LIMBS + 1):
        suffix = suffix + b.loc(COL_Y + LIMBS - i)
        if i < LIMBS:
            high = high + b.loc(COL_Q + i) * suffix
    b.emit(at["high"], high)
    word_table.zero_test(b, at, z, suffix, b.loc(COL_INV), not_zero)

    carry = borrow = 0
    for k in range(LIMBS):
        if k % limbs_per_unit == 0:
            b.unit()
            if k:   # the carries into this unit's first limb, summed again here: registers do not live across units
                carry = bits_sum(b, COL_CARRY + CARRY_BITS * (k - 1), CARRY_BITS)
                borrow = b.loc(COL_BORROW + k - 1)
        xk = bits_value(b, COL_X_BITS + LIMB_BITS * k, LIMB_BITS, at["x_bits"] + LIMB_BITS * k)
        yk = bits_value(b, COL_Y_BITS + LIMB_BITS * k, LIMB_BITS, at["y_bits"] + LIMB_BITS * k)
        qk = bits_value(b, COL_Q_BITS + LIMB_BITS * k, LIMB_BITS, at["q_bits"] + LIMB_BITS * k)
        rk = bits_value(b, COL_R_BITS + LIMB_BITS * k, LIMB_BITS, at["r_bits"] + LIMB_BITS * k)
        dk = bits_value(b, COL_D_BITS + LIMB_BITS * k, LIMB_BITS, at["d_bits"] + LIMB_BITS * k)
        b.emit(at["x_limbs"] + k, b.loc(COL_X + k) - xk)
        b.emit(at["y_limbs"] + k, b.loc(COL_Y + k) - yk)
        b.emit(at["q_limbs"] + k, b.loc(COL_Q + k) - qk)
        conv = 0
        for i in range(k + 1):
            conv = conv + b.loc(COL_Q + i) * b.loc(COL_Y + k - i)
        if k < N_CARRIES:
            out = bits_value(b, COL_CARRY + CARRY_BITS * k, CARRY_BITS, at["carry_bits"] + CARRY_BITS * k)
            b.emit(at["product"] + k, (conv + rk + carry) - (xk + BASE * out))
            carry = out
        else:
            b.emit(at["product"] + k, (conv + rk + carry) - xk)
        borrow = remainder_limb(b, at, k, rk, dk, yk, borrow, COL_BORROW, not_zero)
        b.emit(at["result"] + k, b.loc(COL_RES + k) - not_zero * (is_div * b.loc(COL_Q + k) + is_mod * rk))
    b.emit(at["remainder_top"], not_zero * borrow)
    b.port(g, [b.loc(c) for c in TUPLE_COLS])
    return b


def kernel_layout():
    """bp_arithmetic_div_layout: the column map csrc/arithmetic_div.hip stores by, in LAYOUT's order"""
    return word_table.kernel_layout("bp_arithmetic_div_layout", len(LAYOUT))


def register():
    """Assembles and registers the program (once per process) and returns its air_id.  The column map exists twice, here
    and in the witness kernel: RuntimeError if the two disagree."""
    return word_table.register("arithmetic_div", LAYOUT, "bp_arithmetic_div_layout", program)


def pack_inputs(ops_list):
    """[(op, x, y, exposed), ...] of Python integers -> the [n, 9] uint64 input words of bp_arithmetic_div_trace: word 0
    = op (1 div, 2 mod, else a padding row) | exposed << 8, then the four 64-bit words of x and of y, least significant
    first"""
    return word_table.pack_inputs(ops_list, 2, "x and y")


def unpack_row(trace, i):
    """(op, x, y, q, r, res, g) of row i of a [N_COLS, n] trace (anything indexable as trace[col][row]) as Python
    integers: x, y, res and q from their limb columns, r from its bits"""
    cells = [int(trace[c][i]) for c in range(N_COLS)]
    op = OP_DIV if cells[COL_IS_DIV] else OP_MOD if cells[COL_IS_MOD] else OP_NONE
    return (op, _word(cells, COL_X, LIMB_BITS, LIMBS), _word(cells, COL_Y, LIMB_BITS, LIMBS),
            _word(cells, COL_Q, LIMB_BITS, LIMBS), _word(cells, COL_R_BITS, 1, 256), _word(cells, COL_RES, LIMB_BITS, LIMBS),
            cells[COL_G])
