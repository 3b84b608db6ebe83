"""What the five shipped tables over 256-bit words (arithmetic_div.py, arithmetic_mod.py, arithmetic_shift.py,
arithmetic_sdiv.py, arithmetic_exp.py) share.  All five: the range-checked bit blocks (bits_value, bits_sum), first_index
and the plumbing between such a module, its witness kernel and the library.  The four tables of one operation per row:
the flags of two operations (flags) or of three (flags3, the shift table's) and the zero test.  The quotient / remainder
/ slack tables over 16-bit limbs -- division, modular, signed -- : remainder_limb; the signed table alone the conditional
negation it takes its magnitudes and its result by.  Plain functions over the table's air_program.Builder `b`, its
family bases `at` (name -> first constraint index; the shared families carry the same names in every table) and its
column numbers.  A table module states its column map, LAYOUT, FAMILIES and the part of program() that is its own.

The Builder numbers registers and orders code by the order of Python operations, and a program's id is a digest of its
words: these helpers perform the operations the tables performed before they were factored out, in the same order
(tests/test_program_table_words.py holds the words).
"""
import ctypes as C

import numpy as np

LIMB_BITS = 16
BASE = 1 << LIMB_BITS
EXPOSED = 1 << 8          # bit 8 of input word 0: the row's filter g


# ---- pieces of a program
def bits_value(b, col, n, cidx):
    """the value of the `n` bit columns from `col`, least significant first; constraint cidx + j makes bit j a bit"""
    v = 0
    for j in range(n - 1, -1, -1):
        bit = b.loc(col + j)
        b.emit(cidx + j, bit * bit - bit)
        v = (v + v) + bit
    return v


def bits_sum(b, col, n):
    """the same value without the constraints: a carry summed again in the next unit (registers do not live across
    units), range-checked where it was produced"""
    v = 0
    for j in range(n - 1, -1, -1):
        v = (v + v) + b.loc(col + j)
    return v


def flags(b, at, op_a, op_b, g, z):
    """families flags, one_flag, filter: the two operation flags and z are bits, not both operations, g only on a live row"""
    for j, f in enumerate((op_a, op_b, z)):
        b.emit(at["flags"] + j, f * f - f)
    b.emit(at["one_flag"], op_a * op_b)
    b.emit(at["filter"], g * (1 - op_a - op_b))


def flags3(b, at, flags, g, z):
    """families flags, one_flag, filter for a table of three operations: the flags and z are bits, at most one flag, g
    only on a live row; returns the sum of the flags"""
    for j, f in enumerate(flags + (z,)):
        b.emit(at["flags"] + j, f * f - f)
    live = flags[0] + flags[1] + flags[2]
    b.emit(at["one_flag"], live * (live - 1))
    b.emit(at["filter"], g * (1 - live))
    return live


def zero_test(b, at, z, s, inv, not_zero):
    """family zero: z = [S = 0] for the sum `s` of the divisor's limbs, `inv` its inverse where there is one"""
    b.emit(at["zero"], z * s)
    b.emit(at["zero"] + 1, s * inv - not_zero)


def remainder_limb(b, at, k, rk, dk, yk, borrow_in, col_borrow, not_zero):
    """limb k of r + d + 1 = y, the chain that proves r < y (families borrow_bits, remainder); returns the carry bit out.
    The table closes the chain after limb 15 -- b.emit(at["remainder_top"], not_zero * carry bit) -- where its unit's
    code has always had it."""
    bk = b.loc(col_borrow + k)
    b.emit(at["borrow_bits"] + k, bk * bk - bk)
    b.emit(at["remainder"] + k, not_zero * ((rk + dk + (1 if k == 0 else borrow_in)) - (yk + BASE * bk)))
    return bk


def negation_limb(b, k, sign, vk, wk, col_carry, cidx_bit, cidx):
    """limb k of the conditional negation w = -v mod 2^256 where the bit `sign` is 1, w = v where it is 0: sign (v_k + w_k
    + c_(k-1) - 2^16 c_k) + (1 - sign) (w_k - v_k), stated as (w_k - v_k) + sign (2 v_k + c_(k-1) - 2^16 c_k), the same
    polynomial with one product.  c_k is the bit column col_carry + k (constraint cidx_bit + k), the chain's equation
    constraint cidx + k.  Nothing closes the chain: v + w = 2^256 c_15 with both words below 2^256 leaves c_15 free -- 0
    only for v = w = 0 -- and c_(k-1) is read from its column, so a unit may start at any limb."""
    ck = b.loc(col_carry + k)
    b.emit(cidx_bit + k, ck * ck - ck)
    carry_in = b.loc(col_carry + k - 1) if k else 0
    b.emit(cidx + k, (wk - vk) + sign * ((vk + vk + carry_in) - BASE * ck))


def first_index(families, name):
    """the constraint index at which family `name` of `families` = ((name, count, degree), ...) starts"""
    names = [f[0] for f in families]
    return sum(f[1] for f in families[:names.index(name)])


# ---- the module, its kernel and the library
def kernel_layout(entry_name, n_words):
    """the column map a witness kernel stores by, through its bp_*_layout entry"""
    from ._lib import check, own
    out = (C.c_uint32 * n_words)()
    check(getattr(own(), entry_name)(out, n_words))
    return tuple(int(v) for v in out)


_registered = {}


def register(name, layout, entry_name, program):
    """Assembles and registers program() once per process and returns its air_id; RuntimeError if the kernel's column
    map is not `layout`."""
    if name not in _registered:
        from . import ops
        got = kernel_layout(entry_name, len(layout))
        if got != layout:
            raise RuntimeError("%s: the witness kernel's column map %s is not the program's %s" % (name, got, layout))
        _registered[name] = ops.air_register(program().assemble())
    return _registered[name]


def pack_inputs(rows, k, names):
    """[(op, v_1, ..., v_k, exposed), ...] of Python integers -> [n, 1 + 4 k] uint64: word 0 = op | exposed << 8, then
    the four 64-bit words of each operand, least significant first.  `names` spells the operands in the error."""
    out = np.zeros((len(rows), 1 + 4 * k), dtype=np.uint64)
    for i, (op, *values, exposed) in enumerate(rows):
        if not (0 <= op < 256 and len(values) == k and all(0 <= v < 1 << 256 for v in values)):
            raise ValueError("row %d: op is a byte, %s are 256-bit words" % (i, names))
        out[i, 0] = op | (EXPOSED if exposed else 0)
        for j, v in enumerate(values):
            for w in range(4):
                out[i, 1 + 4 * j + w] = (v >> (64 * w)) & 0xFFFFFFFFFFFFFFFF
    return out


def _word(cells, col, width, n):
    """sum of the `n` values at col, col + 1, ..., each `width` bits wide"""
    return sum(int(cells[col + k]) << (width * k) for k in range(n))
