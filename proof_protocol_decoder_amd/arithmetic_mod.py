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
import ctypes as C

import numpy as np

from .air_program import ALL_ROWS, Builder

OP_NONE, OP_ADDMOD, OP_MULMOD = 0, 1, 2
EXPOSED = 1 << 8          # bit 8 of input word 0: the row's filter g
LIMBS, Q_LIMBS, LIMB_BITS, CARRY_BITS, N_CARRIES = 16, 32, 16, 21, 31
BASE = 1 << LIMB_BITS
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
    return sum(count for _, count, _ in FAMILIES[:FAMILY_INDEX[name]])


def program(cols_per_unit=COLS_PER_UNIT):
    """The table's air_program.Builder: the unit of the flags, the zero test and the high half of q M; then one unit per
    `cols_per_unit` product columns -- columns 0 .. 15 carry limb k of a, b, m, r, d and the result with them, columns
    16 .. 31 only limb k of q --; and the looked port."""
    b = Builder(N_COLS)
    at = {name: b.family(count, ALL_ROWS, degree) for name, count, degree in FAMILIES}
    is_addmod, is_mulmod, g, z = b.loc(COL_IS_ADDMOD), b.loc(COL_IS_MULMOD), b.loc(COL_G), b.loc(COL_Z)
    not_zero = 1 - z

    def bits_value(col, n, cidx):
        v = 0
        for j in range(n - 1, -1, -1):
            bit = b.loc(col + j)
            b.emit(cidx + j, bit * bit - bit)
            v = (v + v) + bit
        return v

    def modulus(j):   # limb j of M = m + z 2^256
        return z if j == LIMBS else b.loc(COL_M + j)

    b.unit()
    for j, f in enumerate((is_addmod, is_mulmod, z)):
        b.emit(at["flags"] + j, f * f - f)
    b.emit(at["one_flag"], is_addmod * is_mulmod)
    b.emit(at["filter"], g * (1 - is_addmod - is_mulmod))
    # T_i = M_16 + M_15 + ... + M_(32 - i): q_i T_i sums the products of q_i that land in columns 32 .. 47
    suffix, high = 0, 0
    for i in range(LIMBS, Q_LIMBS):
        suffix = suffix + modulus(Q_LIMBS - i)
        high = high + b.loc(COL_Q + i) * suffix
    b.emit(at["high"], high)
    s = 0
    for j in range(LIMBS):
        s = s + b.loc(COL_M + j)
    b.emit(at["zero"], z * s)
    b.emit(at["zero"] + 1, s * b.loc(COL_INV) - not_zero)

    carry = borrow = 0
    for k in range(Q_LIMBS):
        if k % cols_per_unit == 0:
            b.unit()
            if k:   # the carry into this unit's first column, summed again here: registers do not live across units
                carry = 0
                for j in range(CARRY_BITS - 1, -1, -1):
                    carry = (carry + carry) + b.loc(COL_CARRY + CARRY_BITS * (k - 1) + j)
                carry = carry - CARRY_OFFSET
                if k < LIMBS:
                    borrow = b.loc(COL_BORROW + k - 1)
        qk = bits_value(COL_Q_BITS + LIMB_BITS * k, LIMB_BITS, at["q_bits"] + LIMB_BITS * k)
        b.emit(at["q_limbs"] + k, b.loc(COL_Q + k) - qk)
        left = right = 0
        for i in range(max(0, k - LIMBS + 1), min(k, LIMBS - 1) + 1):
            left = left + b.loc(COL_A + i) * b.loc(COL_B + k - i)
        left = is_mulmod * left
        for j in range(max(0, k - Q_LIMBS + 1), min(k, LIMBS) + 1):
            right = right + b.loc(COL_Q + k - j) * modulus(j)
        if k < LIMBS:
            ak = bits_value(COL_A_BITS + LIMB_BITS * k, LIMB_BITS, at["a_bits"] + LIMB_BITS * k)
            bk = bits_value(COL_B_BITS + LIMB_BITS * k, LIMB_BITS, at["b_bits"] + LIMB_BITS * k)
            mk = bits_value(COL_M_BITS + LIMB_BITS * k, LIMB_BITS, at["m_bits"] + LIMB_BITS * k)
            rk = bits_value(COL_R_BITS + LIMB_BITS * k, LIMB_BITS, at["r_bits"] + LIMB_BITS * k)
            dk = bits_value(COL_D_BITS + LIMB_BITS * k, LIMB_BITS, at["d_bits"] + LIMB_BITS * k)
            b.emit(at["abm_limbs"] + 3 * k, b.loc(COL_A + k) - ak)
            b.emit(at["abm_limbs"] + 3 * k + 1, b.loc(COL_B + k) - bk)
            b.emit(at["abm_limbs"] + 3 * k + 2, b.loc(COL_M + k) - mk)
            left = left + is_addmod * (b.loc(COL_A + k) + b.loc(COL_B + k))
            right = right + rk
            wk = b.loc(COL_BORROW + k)
            b.emit(at["borrow_bits"] + k, wk * wk - wk)
            b.emit(at["remainder"] + k, not_zero * ((rk + dk + (1 if k == 0 else borrow)) - (mk + BASE * wk)))
            borrow = wk
            b.emit(at["result"] + k, b.loc(COL_RES + k) - not_zero * rk)
        if k < N_CARRIES:
            out = bits_value(COL_CARRY + CARRY_BITS * k, CARRY_BITS, at["carry_bits"] + CARRY_BITS * k) - CARRY_OFFSET
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
    from ._lib import check, own
    out = (C.c_uint32 * len(LAYOUT))()
    check(own().bp_arithmetic_mod_layout(out, len(LAYOUT)))
    return tuple(int(v) for v in out)


_registered = None


def register():
    """Assembles and registers the program (once per process) and returns its air_id.  The column map exists twice, here
    and in the witness kernel: RuntimeError if the two disagree."""
    global _registered
    if _registered is None:
        from . import ops
        got = kernel_layout()
        if got != LAYOUT:
            raise RuntimeError("arithmetic_mod: the witness kernel's column map %s is not the program's %s" % (got, LAYOUT))
        _registered = ops.air_register(program().assemble())
    return _registered


def pack_inputs(ops_list):
    """[(op, a, b, m, exposed), ...] of Python integers -> the [n, 13] uint64 input words of bp_arithmetic_mod_trace:
    word 0 = op (1 addmod, 2 mulmod, else a padding row) | exposed << 8, then the four 64-bit words of a, of b and of m,
    least significant first"""
    out = np.zeros((len(ops_list), 13), dtype=np.uint64)
    for i, (op, a, b, m, exposed) in enumerate(ops_list):
        if not (0 <= op < 256 and all(0 <= v < 1 << 256 for v in (a, b, m))):
            raise ValueError("row %d: op is a byte, a, b and m are 256-bit words" % i)
        out[i, 0] = op | (EXPOSED if exposed else 0)
        for w in range(4):
            out[i, 1 + w] = (a >> (64 * w)) & 0xFFFFFFFFFFFFFFFF
            out[i, 5 + w] = (b >> (64 * w)) & 0xFFFFFFFFFFFFFFFF
            out[i, 9 + w] = (m >> (64 * w)) & 0xFFFFFFFFFFFFFFFF
    return out


def _word(cells, col, width, n):
    """sum of the `n` values at col, col + 1, ..., each `width` bits wide"""
    return sum(int(cells[col + k]) << (width * k) for k in range(n))


def unpack_row(trace, i):
    """(op, a, b, m, q, r, res, g) of row i of a [N_COLS, n] trace (anything indexable as trace[col][row]) as Python
    integers: a, b, m, res and q from their limb columns, r from its bits"""
    cells = [int(trace[c][i]) for c in range(N_COLS)]
    op = OP_ADDMOD if cells[COL_IS_ADDMOD] else OP_MULMOD if cells[COL_IS_MULMOD] else OP_NONE
    return (op, _word(cells, COL_A, LIMB_BITS, LIMBS), _word(cells, COL_B, LIMB_BITS, LIMBS), _word(cells, COL_M, LIMB_BITS, LIMBS),
            _word(cells, COL_Q, LIMB_BITS, Q_LIMBS), _word(cells, COL_R_BITS, 1, 256), _word(cells, COL_RES, LIMB_BITS, LIMBS),
            cells[COL_G])
