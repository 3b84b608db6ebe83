"""The shift table: SHL, SHR and SAR on 256-bit words, one operation per row -- the third constraint program shipped
with the package (air_program.Builder, registered at run time: no built-in air_id) and the witness generator behind
bp_arithmetic_shift_trace (csrc/arithmetic_shift.hip).  AIRS.md section 2, "Shift (a shipped program)", states the layout
and the soundness notes; include/bpg.h the statement and the input words.

    air_id = arithmetic_shift.register()                     # once per process; raises if the kernel's column map differs
    trace = ops.arithmetic_shift_trace(log_n, to_device(arithmetic_shift.pack_inputs([(SHL, s, x, 1), (SAR, s, x, 0)])))
    op, s, x, res, g = arithmetic_shift.unpack_row(trace_on_host, 0)

Operands come in the EVM's order, (shift, value), and the WHOLE 256-bit s decides: z = [s < 256], and a row with z = 0
has res = 0 (SHL, SHR) or sixteen limbs of the sign (SAR).  Below 256 the shift is two steps: by bits 0 .. 3 of s inside
the limbs -- x_k W = lo_k + 2^16 hi_k with W = 2^l or 2^(16 - l), the halves recombined into the committed word y --, then
by bits 4 .. 7 in whole limbs, a one-hot e over the signed offset picking res_k among y's limbs, zero and the fill.  The
one product port exposes (is_shl, is_shr, is_sar, s limbs, x limbs, res limbs) on the rows whose filter column g is 1.
"""
from . import word_table
from .air_program import ALL_ROWS, Builder
from .word_table import BASE, EXPOSED, LIMB_BITS, _word, bits_sum, bits_value, flags3  # noqa: F401 (EXPOSED: the input format's)

OP_NONE, SHL, SHR, SAR = 0, 1, 2, 3
LIMBS, OFFSETS = 16, 31       # e_d for the limb offsets d = -15 .. 15 at COL_E + 15 + d

# ---- the column map (bp_arithmetic_shift_layout states the kernel's)
COL_IS_SHL, COL_IS_SHR, COL_IS_SAR, COL_G, COL_Z, COL_INV, COL_FILL, COL_W = range(8)
COL_S = 8                               # sixteen 16-bit limbs of the shift count s, least significant first
COL_X = COL_S + LIMBS                   # ... of the value x
COL_RES = COL_X + LIMBS                 # ... of the result
COL_Y = COL_RES + LIMBS                 # ... of y, x shifted by bits 0 .. 3 of s
COL_L = COL_Y + LIMBS                   # l_j = [bits 0 .. 3 of s are j]
COL_E = COL_L + LIMBS                   # e_d = [z and the signed limb offset is d]
COL_S_BITS = COL_E + OFFSETS            # bit j of limb k at + 16 k + j, for s, x, lo and hi
COL_X_BITS = COL_S_BITS + LIMBS * LIMB_BITS
COL_LO_BITS = COL_X_BITS + LIMBS * LIMB_BITS
COL_HI_BITS = COL_LO_BITS + LIMBS * LIMB_BITS
N_COLS = COL_HI_BITS + LIMBS * LIMB_BITS   # 1143
LAYOUT = (N_COLS, COL_IS_SHL, COL_IS_SHR, COL_IS_SAR, COL_G, COL_Z, COL_INV, COL_FILL, COL_W, COL_S, COL_X, COL_RES, COL_Y,
          COL_L, COL_E, COL_S_BITS, COL_X_BITS, COL_LO_BITS, COL_HI_BITS)
TUPLE_COLS = (COL_IS_SHL, COL_IS_SHR, COL_IS_SAR) + tuple(range(COL_S, COL_S + 3 * LIMBS))   # the port's 51 elements

# ---- the constraint list: (name, count, degree), all of kind ALL_ROWS, in index order
FAMILIES = (("flags", 4, 2),            # is_shl, is_shr, is_sar, z are bits
            ("one_flag", 1, 2),         # F (F - 1) with F the sum of the three flags
            ("filter", 1, 2),           # g (1 - F)
            ("zero", 2, 2),             # z T, T inv - (1 - z) with T = the limbs 1 .. 15 of s + the value of bits 8 .. 15
            ("operand_bits", 512, 2),   # the bits of s, then of x
            ("operand_limbs", 2 * LIMBS, 1),   # limb column - sum of its bits: s_k at k, x_k at 16 + k
            ("l_bits", LIMBS, 2),
            ("l_hot", 2, 1),            # sum l_j - 1, sum j l_j - (bits 0 .. 3 of s)
            ("e_bits", OFFSETS, 2),
            ("e_hot", 2, 3),            # sum e_d - z, sum d e_d - z (is_shl - is_shr - is_sar) (bits 4 .. 7 of s)
            ("w", 1, 2),                # W - (is_shl sum l_j 2^j + (is_shr + is_sar) sum l_j 2^(16 - j))
            ("fill", 1, 2),             # fill - is_sar (bit 255 of x)
            ("split_bits", 512, 2),     # the bits of the lo_k, then of the hi_k
            ("split", LIMBS, 2),        # x_k W - (lo_k + 2^16 hi_k)
            ("y", LIMBS, 2),            # y_k - is_shl (lo_k + hi_(k-1)) - (is_shr + is_sar) (hi_k + lo_(k+1)) - [k = 15] fill (2^16 - W)
            ("result", LIMBS, 2))       # res_k - sum_d e_d Y_(k-d) - (1 - z) 0xFFFF fill
FAMILY_INDEX = {name: k for k, (name, _, _) in enumerate(FAMILIES)}
# Limbs a unit after the unit of the flags and the two one-hots.  At 2^14 rows on an MI355X one limb a unit (18 units
# with the port's: 9 workgroup rows of two) is 635 us in K5 and 7.00 ms a proof, two (10 rows of one) 646 us and 7.00 ms,
# four (6 rows) 761 us and 7.11 ms (profiles/arithmetic_shift.txt); one also needs 6 registers where the others need 9.
CUTS = (1, 2, 4)
LIMBS_PER_UNIT = 1


def first_index(name):
    """the constraint index at which family `name` starts"""
    return word_table.first_index(FAMILIES, name)


def program(limbs_per_unit=LIMBS_PER_UNIT):
    """The table's air_program.Builder: the unit of the flags, the zero test, the two one-hots, W and the fill; then one
    unit per `limbs_per_unit` limbs -- the bits of s_k and x_k, the split of x_k W, its shares of y_(k-1), y_k, y_(k+1) (an
    index emitted from several units adds up) and res_k --; and the looked port."""
    if limbs_per_unit not in CUTS:
        raise ValueError("limbs_per_unit is one of %s" % (CUTS,))
    b = Builder(N_COLS)
    at = {name: b.family(count, ALL_ROWS, degree) for name, count, degree in FAMILIES}
    is_shl, is_shr, is_sar = b.loc(COL_IS_SHL), b.loc(COL_IS_SHR), b.loc(COL_IS_SAR)
    g, z, fill, w = b.loc(COL_G), b.loc(COL_Z), b.loc(COL_FILL), b.loc(COL_W)
    right = is_shr + is_sar

    b.unit()
    flags3(b, at, (is_shl, is_shr, is_sar), g, z)
    t = bits_sum(b, COL_S_BITS + 8, 8)
    for k in range(1, LIMBS):
        t = t + b.loc(COL_S + k)
    word_table.zero_test(b, at, z, t, b.loc(COL_INV), 1 - z)
    b.emit(at["fill"], fill - is_sar * b.loc(COL_X_BITS + 255))
    hot = index = up = down = 0
    for j in range(LIMBS):
        lj = b.loc(COL_L + j)
        b.emit(at["l_bits"] + j, lj * lj - lj)
        hot, index = hot + lj, (index + j * lj if j else index)
        up, down = up + (1 << j) * lj, down + (1 << (LIMB_BITS - j)) * lj
    b.emit(at["l_hot"], hot - 1)
    b.emit(at["l_hot"] + 1, index - bits_sum(b, COL_S_BITS, 4))
    b.emit(at["w"], w - is_shl * up)     # two emits: a leaf lives to its last use in an emit, and both sums load every l_j
    b.emit(at["w"], 0 - right * down)
    hot = index = 0
    for d in range(-15, 16):
        ed = b.loc(COL_E + 15 + d)
        b.emit(at["e_bits"] + 15 + d, ed * ed - ed)
        hot, index = hot + ed, (index + d * ed if d else index)
    b.emit(at["e_hot"], hot - z)
    b.emit(at["e_hot"] + 1, index - z * (is_shl - right) * bits_sum(b, COL_S_BITS + 4, 4))

    for k in range(LIMBS):
        if k % limbs_per_unit == 0:
            b.unit()
        sk = bits_value(b, COL_S_BITS + LIMB_BITS * k, LIMB_BITS, at["operand_bits"] + LIMB_BITS * k)
        xk = bits_value(b, COL_X_BITS + LIMB_BITS * k, LIMB_BITS, at["operand_bits"] + 256 + LIMB_BITS * k)
        b.emit(at["operand_limbs"] + k, b.loc(COL_S + k) - sk)
        b.emit(at["operand_limbs"] + LIMBS + k, b.loc(COL_X + k) - xk)
        lo = bits_value(b, COL_LO_BITS + LIMB_BITS * k, LIMB_BITS, at["split_bits"] + LIMB_BITS * k)
        hi = bits_value(b, COL_HI_BITS + LIMB_BITS * k, LIMB_BITS, at["split_bits"] + 256 + LIMB_BITS * k)
        b.emit(at["split"] + k, b.loc(COL_X + k) * w - (lo + BASE * hi))
        # y_k = is_shl (lo_k + hi_(k-1)) + right (hi_k + lo_(k+1)): this limb's halves go to three constraints
        b.emit(at["y"] + k, b.loc(COL_Y + k) - (is_shl * lo + right * hi))
        if k + 1 < LIMBS:
            b.emit(at["y"] + k + 1, 0 - is_shl * hi)
        else:
            b.emit(at["y"] + k, 0 - fill * (BASE - w))
        if k:
            b.emit(at["y"] + k - 1, 0 - right * lo)
        # res_k = sum_d e_d Y_(k-d): y_(k-d) for k - 15 <= d <= k, the fill above limb 15, zero below limb 0
        moved = above = 0
        for d in range(-15, k + 1):
            if k - d < LIMBS:
                moved = moved + b.loc(COL_E + 15 + d) * b.loc(COL_Y + k - d)
            else:
                above = above + b.loc(COL_E + 15 + d)
        b.emit(at["result"] + k, b.loc(COL_RES + k) - (moved + (BASE - 1) * fill * (above + (1 - z))))
    b.port(g, [b.loc(c) for c in TUPLE_COLS])
    return b


def kernel_layout():
    """bp_arithmetic_shift_layout: the column map csrc/arithmetic_shift.hip stores by, in LAYOUT's order"""
    return word_table.kernel_layout("bp_arithmetic_shift_layout", len(LAYOUT))


def register():
    """Assembles and registers the program (once per process) and returns its air_id.  The column map exists twice, here
    and in the witness kernel: RuntimeError if the two disagree."""
    return word_table.register("arithmetic_shift", LAYOUT, "bp_arithmetic_shift_layout", program)


def pack_inputs(ops_list):
    """[(op, s, x, exposed), ...] of Python integers -> the [n, 9] uint64 input words of bp_arithmetic_shift_trace: word 0
    = op (1 shl, 2 shr, 3 sar, else a padding row) | exposed << 8, then the four 64-bit words of the shift count s and of
    the value x, least significant first"""
    return word_table.pack_inputs(ops_list, 2, "s and x")


def unpack_row(trace, i):
    """(op, s, x, res, g) of row i of a [N_COLS, n] trace (anything indexable as trace[col][row]) as Python integers,
    the three words from their limb columns"""
    cells = [int(trace[c][i]) for c in range(COL_Y)]
    op = SHL if cells[COL_IS_SHL] else SHR if cells[COL_IS_SHR] else SAR if cells[COL_IS_SAR] else OP_NONE
    return (op, _word(cells, COL_S, LIMB_BITS, LIMBS), _word(cells, COL_X, LIMB_BITS, LIMBS),
            _word(cells, COL_RES, LIMB_BITS, LIMBS), cells[COL_G])
