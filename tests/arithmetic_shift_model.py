"""An independent model of the shift table (proof_protocol_decoder_amd/arithmetic_shift.py, csrc/arithmetic_shift.hip),
shared by tests/test_arithmetic_shift.py and tests/test_gpu_arithmetic_shift.py.  It works from the statement in
include/bpg.h and the column list in AIRS.md section 2 ("Shift (a shipped program)") over Python integers (<<, >>, %):
it imports nothing of the package, so the column map below is a third statement of it and the tests compare it with the
package's.  The limb helpers, the writer of a row's bit blocks, the model trace and the forged row are
tests/word_table_model.py's, as independent as this file.

    w = honest(op, s, x, exposed)     the witness of one operation: a dict of what a row holds
    cells(w)                          the 1143 cells of its row
    CATALOGUE                         wrong witnesses, each otherwise consistent: (name, operation, forge, families broken)
"""
import random

import word_table_model as base
from word_table_model import B, M256, P, limbs, word  # noqa: F401 (the tests read them here)

NONE, SHL, SHR, SAR = 0, 1, 2, 3
LIVE = (SHL, SHR, SAR)

# AIRS.md section 2: eight single columns, four blocks of 16 limbs, the one-hots l (16) and e (31), four bit blocks
IS_SHL, IS_SHR, IS_SAR, G, Z, INV, FILL, W = range(8)
S, X, RES, Y = 8, 24, 40, 56
L, E = 72, 88
S_BITS, X_BITS, LO_BITS, HI_BITS, N_COLS = 119, 375, 631, 887, 1143
# the families in constraint order, with their sizes
FAMILIES = [("flags", 4), ("one_flag", 1), ("filter", 1), ("zero", 2), ("operand_bits", 512), ("operand_limbs", 32),
            ("l_bits", 16), ("l_hot", 2), ("e_bits", 31), ("e_hot", 2), ("w", 1), ("fill", 1), ("split_bits", 512),
            ("split", 16), ("y", 16), ("result", 16)]
N_CONSTRAINTS = sum(c for _, c in FAMILIES)   # 1165


def statement(op, s, x):
    """res of a live operation, as include/bpg.h states it: over the integers, the whole s deciding"""
    sign = x >> 255
    if op == SHL:
        return (x << s) & M256 if s < 256 else 0
    if op == SHR:
        return x >> s if s < 256 else 0
    assert op == SAR
    if s >= 256:
        return sign * M256
    return (x >> s) + sign * ((1 << 256) - (1 << (256 - s)))


def honest(op, s, x, exposed):
    """The witness the statement asks for.  A padding row (op none of SHL, SHR, SAR) ignores s, x and exposed."""
    if op not in LIVE:
        s = x = exposed = 0
    w = {"is_shl": int(op == SHL), "is_shr": int(op == SHR), "is_sar": int(op == SAR), "g": int(bool(exposed)),
         "z": int(s < 256), "fill": int(op == SAR) * (x >> 255),
         "sl": limbs(s), "xl": limbs(x),        # the limb columns
         "sb": s, "xb": x,                      # the words the bit columns spell
         "fixed": set()}                        # what a forgery states itself: chains() leaves it alone
    chains(w)
    assert word(w["resl"]) == (statement(op, s, x) if op in LIVE else 0), (op, s, hex(x))
    assert all(0 <= v < B for v in w["y"] + w["lo"] + w["hi"])
    return w


def chains(w):
    """(Re)derives what follows from the rest of the witness, in the order the constraints tie it: the inverse of the
    zero test, the one-hots l and e, W, the split of every x_k W, y and the result -- each unless the forgery has fixed
    it.  A forged witness stays consistent wherever it can."""
    fixed = w["fixed"]
    right = w["is_shr"] + w["is_sar"]
    t = sum(w["sl"][1:]) + ((w["sb"] >> 8) & 0xFF)
    w["inv"] = pow(t, P - 2, P) if t % P and not w["z"] else 0
    if "l" not in fixed:
        w["l"] = [int(j == w["sb"] & 15) for j in range(16)]
    if "e" not in fixed:
        d = (w["is_shl"] - right) * ((w["sb"] >> 4) & 15)
        assert -15 <= d <= 15
        w["e"] = [int(bool(w["z"]) and k == 15 + d) for k in range(31)]
    if "W" not in fixed:
        w["W"] = w["is_shl"] * sum(l << j for j, l in enumerate(w["l"])) + right * sum(l << (16 - j) for j, l in enumerate(w["l"]))
    if "lo" not in fixed:
        products = [xk * w["W"] for xk in w["xl"]]
        w["lo"], w["hi"] = [v & 0xFFFF for v in products], [v >> 16 for v in products]
    lo, hi = w["lo"], w["hi"]
    if "y" not in fixed:
        w["y"] = [w["is_shl"] * (lo[k] + (hi[k - 1] if k else 0)) + right * (hi[k] + (lo[k + 1] if k < 15 else 0))
                  for k in range(16)]
        w["y"][15] += w["fill"] * (B - w["W"])
    if "resl" not in fixed:
        ones = 0xFFFF * w["fill"]

        def moved(m):   # Y_m: a limb of y, zero below it, the fill above it
            return 0 if m < 0 else w["y"][m] if m < 16 else ones
        w["resl"] = [sum(w["e"][15 + d] * moved(k - d) for d in range(-15, 16)) + (1 - w["z"]) * ones for k in range(16)]
    return w


def cells(w):
    """the 1143 cells of the row, as Python integers below p"""
    row = [0] * N_COLS
    row[IS_SHL], row[IS_SHR], row[IS_SAR], row[G], row[Z] = w["is_shl"], w["is_shr"], w["is_sar"], w["g"], w["z"]
    row[INV], row[FILL], row[W] = w["inv"], w["fill"], w["W"]
    for k in range(16):
        row[S + k], row[X + k], row[RES + k], row[Y + k], row[L + k] = w["sl"][k], w["xl"][k], w["resl"][k], w["y"][k], w["l"][k]
    for k in range(31):
        row[E + k] = w["e"][k]
    spelt = dict(w, lob=word(w["lo"]), hib=word(w["hi"]), carry=[])
    blocks = ((S_BITS, "sb", 256), (X_BITS, "xb", 256), (LO_BITS, "lob", 256), (HI_BITS, "hib", 256))
    return base.put_blocks(row, spelt, blocks, 0, 0)


def trace_of(ops):
    """[1143, len(ops)] uint64: the model trace of a list of (op, s, x, exposed)"""
    return base.trace_of(honest, cells, ops)


# ---------------------------------------------------------------------------------------------- the edge list
MAX = M256
TOP = 1 << 255
G1 = 0xFEDC << 240 | 0x13579BDF2468ACE << 120 | 0x9999 << 16 | 0x7      # a negative word
G2 = 0x40DE << 240 | 0xFFFF0000FFFF << 96 | 0x1235                        # a positive one
HIGH_BYTE = 0x300                # low byte zero, the high byte of limb 0 set: 768, not 0
LIMB_ONE = (1 << 16) + 5         # a small low byte under a set limb 1: not 5
# (s, x): twelve shift counts against the negative word, then the values x at counts that move them
EDGE_PAIRS = [(0, G1), (1, G1), (15, G1), (16, G1), (17, G1), (255, G1), (256, G1), (257, G1), (HIGH_BYTE, G1),
              (LIMB_ONE, G1), (TOP, G1), (MAX, G1),
              (4, 0), (200, 1), (1, TOP), (255, TOP), (3, TOP - 1), (100, MAX), (255, MAX), (240, G2)]
PADDING = [(NONE, MAX, G1, 1), (4, 1 << 200 | 5, MAX, 1), (0xFF, 7, TOP, 0), (0x80, MAX, MAX, 1)]   # operand words to ignore
PADDING_ROWS = (9, 21, 22, 23)   # where edge_ops() has them


def random_ops(n, seed):
    """seeded operations: x of every length from 0 to 256 bits; half the rows draw s below 256, the others a word of any
    length; a padding row now and then"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        s = rng.randrange(256) if rng.random() < 0.5 else rng.getrandbits(rng.randint(0, 256))
        out.append((rng.choice((SHL, SHL, SHR, SHR, SAR, SAR, SAR, NONE, 7)), s, rng.getrandbits(rng.randint(0, 256)), rng.randint(0, 1)))
    return out


def edge_ops():
    """2^5 rows: every edge pair once, the operation going round SHL, SHR, SAR (so SAR meets the negative word at 15, 255,
    0x300 and 2^256 - 1), the exposed bit changing every second row; a padding row at 9, three more after the pairs;
    random operations"""
    ops = [((SHL, SHR, SAR)[k % 3], s, x, (k // 2) % 2) for k, (s, x) in enumerate(EDGE_PAIRS)]
    ops = ops[:9] + PADDING[:1] + ops[9:] + PADDING[1:]
    return ops + random_ops(32 - len(ops), 0x5F70)


def edge_ops_full():
    """2^7 rows: every edge pair under all three flags, exposed and not; the padding rows; random operations"""
    ops = [(op, s, x, e) for s, x in EDGE_PAIRS for op in LIVE for e in (1, 0)] + PADDING
    return ops + random_ops(128 - len(ops), 0x5F71)


# ---------------------------------------------------------------------------------------------- wrong witnesses
def _fix(w, **stated):
    w.update(stated)
    w["fixed"] |= set(stated)


def _two_bits_in_l(w):
    """l_1 = l_2 = 1 for a count whose low four bits are 3: the weighted sum is right, the plain sum is 2"""
    assert w["sb"] & 15 == 3
    _fix(w, l=[int(j in (1, 2)) for j in range(16)])


def _e_at(d):
    def forge(w):
        _fix(w, e=[int(k == 15 + d) for k in range(31)])
    return forge


def _z_on_a_big_shift(w):
    """z = 1 with s >= 256, and everything else in line with it: the count masked to eight bits"""
    assert w["sb"] >= 256
    w.update(z=1)


def _no_z_on_a_small_shift(w):
    assert w["sb"] < 256
    w.update(z=0)


def _w_of_the_other_direction(w):
    assert w["is_shl"] and w["sb"] & 15
    _fix(w, W=1 << (16 - (w["sb"] & 15)))


def _split_off_by_one(w):
    """lo_3 + 1: a multiple of 2^11 plus one, still 16 bits"""
    lo = list(w["lo"])
    lo[3] += 1
    assert lo[3] < B
    _fix(w, lo=lo, hi=w["hi"])


def _wrong_y(w):
    y = list(w["y"])
    y[2] ^= 1
    _fix(w, y=y)


def _fill(value):
    def forge(w):
        assert w["fill"] != value
        w.update(fill=value)
    return forge


def _masked_result(w):
    """res of the count's low byte, the rest of the row honest"""
    op = SHL if w["is_shl"] else SHR if w["is_shr"] else SAR
    assert w["sb"] >= 256
    _fix(w, resl=limbs(statement(op, w["sb"] & 0xFF, w["xb"])))


def _two_flags(w):
    """SHL and SHR at once, both directions' W, g = 0: only the flag pair is wrong"""
    w.update(is_shr=1, g=0)


def _exposed_padding(w):
    w.update(g=1)


def _flag_no_bit(w):
    """is_shl = 2 and is_shr = -1: their sum is 1, so nothing but the two bit constraints sees it (x = 0)"""
    assert w["xb"] == 0 and (w["sb"] >> 4) == 0
    w.update(is_shl=2, is_shr=-1)


def _non_bit(col):
    def forge(w):
        """bits (1, 0) of a limb that is 2, written as (0, 2): the same value"""
        w["poke"] = {col: 2, col + 1: 0}
    return forge


def _fat_limb(w):
    """limb column x_0 holds x_0 + 2^16 and x_1 one less: the same integer x, and with W = 1 the split follows it"""
    xl = list(w["xl"])
    assert xl[1] > 0 and w["sb"] & 15 == 0
    xl[0], xl[1] = xl[0] + B, xl[1] - 1
    w.update(xl=xl, xb=w["xb"] - B)   # the bits spell (x_0, x_1 - 1, ...): only limb 0 differs from its column


def _l_no_bit(w):
    """l_2 = 2, l_1 = -1 for a count of 3: both sums are right (x = 0)"""
    assert w["sb"] & 15 == 3 and w["xb"] == 0
    _fix(w, l=[{2: 2, 1: -1}.get(j, 0) for j in range(16)])


def _e_no_bit(w):
    """e_2 = 2, e_1 = -1 for a left shift by three limbs: both sums are right (x = 0)"""
    assert w["is_shl"] and w["sb"] == 0x30 and w["xb"] == 0
    _fix(w, e=[{17: 2, 16: -1}.get(k, 0) for k in range(31)])


_S_LIMB_5 = 2 << 80 | 3          # limb 5 of the count is 2
# (name, the honest operation, the forgery, the families that break -- nothing else may)
CATALOGUE = [("two_bits_in_l", (SHL, 3, G1, 1), _two_bits_in_l, {"l_hot"}),
             ("e_at_another_offset", (SHR, 0x25, G1, 1), _e_at(-3), {"e_hot"}),
             ("e_on_a_big_shift", (SHL, 0x125, G1, 1), _e_at(2), {"e_hot"}),
             ("z_on_a_big_shift", (SHL, 0x100, G1, 1), _z_on_a_big_shift, {"zero"}),
             ("no_z_on_a_small_shift", (SHR, 5, G1, 1), _no_z_on_a_small_shift, {"zero"}),
             ("w_of_the_other_direction", (SHL, 5, G1, 1), _w_of_the_other_direction, {"w"}),
             ("split_off_by_one", (SHR, 5, G1, 0), _split_off_by_one, {"split"}),
             ("wrong_y", (SHL, 5, G1, 1), _wrong_y, {"y"}),
             ("fill_under_shr", (SHR, 5, G1, 1), _fill(1), {"fill"}),
             ("no_fill_under_sar_of_a_negative_word", (SAR, 5, G1, 1), _fill(0), {"fill"}),
             ("result_of_the_masked_shift", (SAR, LIMB_ONE, G1, 1), _masked_result, {"result"}),
             ("two_flags", (SHL, 3, 0x1234, 0), _two_flags, {"one_flag"}),
             ("exposed_padding_row", (NONE, 0, 0, 0), _exposed_padding, {"filter"}),
             ("flag_that_is_no_bit", (SHL, 3, 0, 1), _flag_no_bit, {"flags"}),
             ("non_bit_in_s", (SHR, _S_LIMB_5, G1, 1), _non_bit(S_BITS + 80), {"operand_bits"}),
             ("limb_of_two_to_the_16", (SHL, 16, G1, 1), _fat_limb, {"operand_limbs"}),
             ("non_bit_in_l", (SHL, 3, 0, 1), _l_no_bit, {"l_bits"}),
             ("non_bit_in_e", (SHL, 0x30, 0, 0), _e_no_bit, {"e_bits"}),
             ("non_bit_in_lo", (SHL, 1, 1, 1), _non_bit(LO_BITS), {"split_bits"})]


def forged(entry):
    """the cells of a catalogue entry's row"""
    return base.forged(honest, chains, cells, entry)


def family_of(index):
    return base.family_of(FAMILIES, index)
