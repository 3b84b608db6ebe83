"""The modular table: ADDMOD and MULMOD on 256-bit words, one operation per row -- the second constraint program shipped
with the package (air_program.Builder, registered at run time: no built-in air_id) and the witness generator behind
bp_arithmetic_mod_trace (csrc/arithmetic_mod.hip).  AIRS.md section 2, "Modular (a shipped program)", states the layout
and the soundness notes; include/bpg.h the statement and the input words.

    air_id = arithmetic_mod.register()                       # once per process; raises if the kernel's column map differs
    trace = ops.arithmetic_mod_trace(log_n, to_device(arithmetic_mod.pack_inputs([(ADDMOD, a, b, m, 1), (MULMOD, a, b, m, 0)])))
    op, a, b, m, q, r, res, g = arithmetic_mod.unpack_row(trace_on_host, 0)

Every row proves U = q M + r over the integers -- U = a + b (257 bits) or a b (512 bits), never reduced modulo 2^256 on
the way, M = m + z 2^256 with z = [m = 0] --, r < m unless m = 0, and res = (1 - z) r.  The one product port exposes
(is_addmod, is_mulmod, a limbs, b limbs, m limbs, res limbs) on the rows whose filter column g is 1.
"""
from . import word_table
from .air_program import ALL_ROWS, Builder
from .word_table import BASE, EXPOSED, LIMB_BITS, _word, bits_sum, bits_value, remainder_limb

OP_NONE, OP_ADDMOD, OP_MULMOD = 0, 1, 2
LIMBS, Q_LIMBS, CARRY_BITS, N_CARRIES = 16, 32, 21, 31
CARRY_OFFSET = 1 << 20    # a carry column group holds c_k + 2^20: the carries are signed, |c_k| < 2^20

# ---- the column map (bp_arithmetic_mod_layout states the kernel's)
COL_IS_ADDMOD, COL_IS_MULMOD, COL_G, COL_Z, COL_INV = 0, 1, 2, 3, 4
COL_A = 5                               # sixteen 16-bit limbs of a, least significant first
COL_B = COL_A + LIMBS                   # ... of b
COL_M = COL_B + LIMBS                   # ... of the modulus
COL_RES = COL_M + LIMBS                 # ... of the result
COL_Q = COL_RES + LIMBS                 # the 32 limbs of the quotient
COL_A_BITS = COL_Q + Q_LIMBS            # bit j of limb k at + 16 k + j, for a, b, m, q (512 bits), r and the slack d = m - r - 1
COL_B_BITS = COL_A_BITS + LIMBS * LIMB_BITS
COL_M_BITS = COL_B_BITS + LIMBS * LIMB_BITS
COL_Q_BITS = COL_M_BITS + LIMBS * LIMB_BITS
COL_R_BITS = COL_Q_BITS + Q_LIMBS * LIMB_BITS
COL_D_BITS = COL_R_BITS + LIMBS * LIMB_BITS
COL_CARRY = COL_D_BITS + LIMBS * LIMB_BITS   # bit j of c_k + 2^20, the carry out of product column k (k < 31), at + 21 k + j
COL_BORROW = COL_CARRY + N_CARRIES * CARRY_BITS   # the carry bit out of limb k of r + d + 1
N_COLS = COL_BORROW + LIMBS             # 2560
LAYOUT = (N_COLS, COL_IS_ADDMOD, COL_IS_MULMOD, COL_G, COL_Z, COL_INV, COL_A, COL_B, COL_M, COL_RES, COL_Q, COL_A_BITS,
          COL_B_BITS, COL_M_BITS, COL_Q_BITS, COL_R_BITS, COL_D_BITS, COL_CARRY, CARRY_BITS, CARRY_OFFSET, COL_BORROW)
TUPLE_COLS = (COL_IS_ADDMOD, COL_IS_MULMOD) + tuple(range(COL_A, COL_A + 4 * LIMBS))   # the port's 66 elements

# ---- the constraint list: (name, count, degree), all of kind ALL_ROWS, in index order
FAMILIES = (("flags", 3, 2),            # is_addmod, is_mulmod, z are bits
            ("one_flag", 1, 2),         # is_addmod is_mulmod
            ("filter", 1, 2),           # g (1 - is_addmod - is_mulmod)
            ("zero", 2, 2),             # z S, S inv - (1 - z) with S = sum of m's limbs
            ("high", 1, 2),             # sum_{i + j >= 32} q_i M_j, M_16 = z
            ("a_bits", 256, 2), ("b_bits", 256, 2), ("m_bits", 256, 2), ("q_bits", 512, 2), ("r_bits", 256, 2), ("d_bits", 256, 2),
            ("carry_bits", N_CARRIES * CARRY_BITS, 2), ("borrow_bits", LIMBS, 2),
            ("abm_limbs", 3 * LIMBS, 1),   # limb column - sum of its bits: a_k at 3 k, b_k at 3 k + 1, m_k at 3 k + 2
            ("q_limbs", Q_LIMBS, 1),
            ("product", Q_LIMBS, 3),    # L_k - R_k + c_{k-1} - 2^16 c_k  (no c_31)
            ("remainder", LIMBS, 2),    # (1 - z) (r_k + d_k + [k = 0] + b_{k-1} - m_k - 2^16 b_k)
            ("remainder_top", 1, 2),    # (1 - z) b_15
            ("result", LIMBS, 2))       # res_k - (1 - z) r_k
FAMILY_INDEX = {name: k for k, (name, _, _) in enumerate(FAMILIES)}
# One product column a unit (33 units with the first): at 2^14 rows a proof takes 13.63 ms on an MI355X so, 13.88 ms with
# two columns a unit and 13.90 with four (profiles/arithmetic_mod.txt) -- K5 packs the units into at most 16 workgroup
# rows at that height: 34 units make 12 rows of three, 18 units only 9 rows of two.
COLS_PER_UNIT = 1


def first_index(name):
    """the constraint index at which family `name` starts"""
    return word_table.first_index(FAMILIES, name)


def program(cols_per_unit=COLS_PER_UNIT):
    """The table's air_program.Builder: the unit of the flags, the zero test and the high half of q M; then one unit per
    `cols_per_unit` product columns -- columns 0 .. 15 carry limb k of a, b, m, r, d and the result with them, columns
    16 .. 31 only limb k of q --; and the looked port."""
    b = Builder(N_COLS)
    at = {name: b.family(count, ALL_ROWS, degree) for name, count, degree in FAMILIES}
    is_addmod, is_mulmod, g, z = b.loc(COL_IS_ADDMOD), b.loc(COL_IS_MULMOD), b.loc(COL_G), b.loc(COL_Z)
    not_zero = 1 - z

    def modulus(j):   # limb j of M = m + z 2^256
        return z if j == LIMBS else b.loc(COL_M + j)

    b.unit()
    word_table.flags(b, at, is_addmod, is_mulmod, g, z)
    # T_i = M_16 + M_15 + ... + M_(32 - i): q_i T_i sums the products of q_i that land in columns 32 .. 47
    suffix, high = 0, 0
    for i in range(LIMBS, Q_LIMBS):
        suffix = suffix + modulus(Q_LIMBS - i)
        high = high + b.loc(COL_Q + i) * suffix
    b.emit(at["high"], high)
    s = 0
    for j in range(LIMBS):
        s = s + b.loc(COL_M + j)
    word_table.zero_test(b, at, z, s, b.loc(COL_INV), not_zero)

    carry = borrow = 0
    for k in range(Q_LIMBS):
        if k % cols_per_unit == 0:
            b.unit()
            if k:   # the carry into this unit's first column, summed again here: registers do not live across units
                carry = bits_sum(b, COL_CARRY + CARRY_BITS * (k - 1), CARRY_BITS) - CARRY_OFFSET
                if k < LIMBS:
                    borrow = b.loc(COL_BORROW + k - 1)
        qk = bits_value(b, COL_Q_BITS + LIMB_BITS * k, LIMB_BITS, at["q_bits"] + LIMB_BITS * k)
        b.emit(at["q_limbs"] + k, b.loc(COL_Q + k) - qk)
        left = right = 0
        for i in range(max(0, k - LIMBS + 1), min(k, LIMBS - 1) + 1):
            left = left + b.loc(COL_A + i) * b.loc(COL_B + k - i)
        left = is_mulmod * left
        for j in range(max(0, k - Q_LIMBS + 1), min(k, LIMBS) + 1):
            right = right + b.loc(COL_Q + k - j) * modulus(j)
        if k < LIMBS:
            ak = bits_value(b, COL_A_BITS + LIMB_BITS * k, LIMB_BITS, at["a_bits"] + LIMB_BITS * k)
            bk = bits_value(b, COL_B_BITS + LIMB_BITS * k, LIMB_BITS, at["b_bits"] + LIMB_BITS * k)
            mk = bits_value(b, COL_M_BITS + LIMB_BITS * k, LIMB_BITS, at["m_bits"] + LIMB_BITS * k)
            rk = bits_value(b, COL_R_BITS + LIMB_BITS * k, LIMB_BITS, at["r_bits"] + LIMB_BITS * k)
            dk = bits_value(b, COL_D_BITS + LIMB_BITS * k, LIMB_BITS, at["d_bits"] + LIMB_BITS * k)
            b.emit(at["abm_limbs"] + 3 * k, b.loc(COL_A + k) - ak)
            b.emit(at["abm_limbs"] + 3 * k + 1, b.loc(COL_B + k) - bk)
            b.emit(at["abm_limbs"] + 3 * k + 2, b.loc(COL_M + k) - mk)
            left = left + is_addmod * (b.loc(COL_A + k) + b.loc(COL_B + k))
            right = right + rk
            borrow = remainder_limb(b, at, k, rk, dk, mk, borrow, COL_BORROW, not_zero)
            b.emit(at["result"] + k, b.loc(COL_RES + k) - not_zero * rk)
        if k < N_CARRIES:
            out = bits_value(b, COL_CARRY + CARRY_BITS * k, CARRY_BITS, at["carry_bits"] + CARRY_BITS * k) - CARRY_OFFSET
            b.emit(at["product"] + k, (left + carry) - (right + BASE * out))
            carry = out
        else:
            b.emit(at["product"] + k, (left + carry) - right)
        if k == LIMBS - 1:
            b.emit(at["remainder_top"], not_zero * borrow)
    b.port(g, [b.loc(c) for c in TUPLE_COLS])
    return b


def kernel_layout():
    """bp_arithmetic_mod_layout: the column map csrc/arithmetic_mod.hip stores by, in LAYOUT's order"""
    return word_table.kernel_layout("bp_arithmetic_mod_layout", len(LAYOUT))


def register():
    """Assembles and registers the program (once per process) and returns its air_id.  The column map exists twice, here
    and in the witness kernel: RuntimeError if the two disagree."""
    return word_table.register("arithmetic_mod", LAYOUT, "bp_arithmetic_mod_layout", program)


def pack_inputs(ops_list):
    """[(op, a, b, m, exposed), ...] of Python integers -> the [n, 13] uint64 input words of bp_arithmetic_mod_trace:
    word 0 = op (1 addmod, 2 mulmod, else a padding row) | exposed << 8, then the four 64-bit words of a, of b and of m,
    least significant first"""
    return word_table.pack_inputs(ops_list, 3, "a, b and m")


def unpack_row(trace, i):
    """(op, a, b, m, q, r, res, g) of row i of a [N_COLS, n] trace (anything indexable as trace[col][row]) as Python
    integers: a, b, m, res and q from their limb columns, r from its bits"""
    cells = [int(trace[c][i]) for c in range(N_COLS)]
    op = OP_ADDMOD if cells[COL_IS_ADDMOD] else OP_MULMOD if cells[COL_IS_MULMOD] else OP_NONE
    return (op, _word(cells, COL_A, LIMB_BITS, LIMBS), _word(cells, COL_B, LIMB_BITS, LIMBS), _word(cells, COL_M, LIMB_BITS, LIMBS),
            _word(cells, COL_Q, LIMB_BITS, Q_LIMBS), _word(cells, COL_R_BITS, 1, 256), _word(cells, COL_RES, LIMB_BITS, LIMBS),
            cells[COL_G])
