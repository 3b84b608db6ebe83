"""An independent model of the signed table (proof_protocol_decoder_amd/arithmetic_sdiv.py, csrc/arithmetic_sdiv.hip),
shared by tests/test_arithmetic_sdiv.py and tests/test_gpu_arithmetic_sdiv.py.  It works from the statement in
include/bpg.h and the column list in AIRS.md section 2 ("Signed (a shipped program)") over Python integers (divmod on
the magnitudes): it imports nothing of the package, so the column map below is a third statement of it and the tests
compare it with the package's.  The limb helpers, the carry bits of r + d + 1, the writer of a row's bit blocks, the model
trace and the forged row are tests/word_table_model.py's, as independent as this file; the carry bits of a negation, the
mirror of word_table.negation_limb, are stated here.

    w = honest(op, x, y, exposed)     the witness of one operation: a dict of what a row holds
    cells(w)                          the 2499 cells of its row
    CATALOGUE                         wrong witnesses, each otherwise consistent: (name, operation, forge, families broken)
"""
import random

import word_table_model as base
from word_table_model import B, M256, P, limbs, word  # noqa: F401 (the tests read them here)

NONE, SDIV, SMOD = 0, 1, 2
LIVE = (SDIV, SMOD)
CARRY_BITS = 19

# AIRS.md section 2: six single columns, six limb blocks, eight bit blocks, 15 carries of 19 bits, the 16 carry bits of
# r + d + 1 and of the three negations
IS_SDIV, IS_SMOD, G, Z, INV, NEG = range(6)
X, Y, RES, Q, AY, M = 6, 22, 38, 54, 70, 86
X_BITS, Y_BITS, RES_BITS, AX_BITS, AY_BITS, Q_BITS, R_BITS, D_BITS = 102, 358, 614, 870, 1126, 1382, 1638, 1894
CARRY, BORROW, X_CHAIN, Y_CHAIN, RES_CHAIN, N_COLS = 2150, 2435, 2451, 2467, 2483, 2499
# the families in constraint order, with their sizes
FAMILIES = [("flags", 3), ("one_flag", 1), ("filter", 1), ("zero", 2), ("high", 1), ("neg", 1), ("operand_bits", 768),
            ("magnitude_bits", 512), ("core_bits", 768), ("carry_bits", 285), ("borrow_bits", 16), ("chain_bits", 48),
            ("limbs", 80), ("magnitude", 32), ("product", 16), ("remainder", 16), ("remainder_top", 1), ("m", 16),
            ("result", 16)]
N_CONSTRAINTS = sum(c for _, c in FAMILIES)   # 2583


def to_word(v):
    """the two's-complement word of a signed integer in [-2^255, 2^255)"""
    assert -(1 << 255) <= v < 1 << 255
    return v & M256


def magnitude(v):
    """|V| of the word v = V mod 2^256: 2^255 for the most negative one"""
    return (1 << 256) - v if v >> 255 else v


def negation_chain(sign, v_limbs, w_limbs):
    """the mirror of word_table.negation_limb: the sixteen carry bits of v + w, limb by limb, where the word is negated
    (v + w = 2^256 c_15); all zero where `sign` is 0 and w = v"""
    carries, c = [], 0
    for vk, wk in zip(v_limbs, w_limbs):
        c = (vk + wk + c) >> 16 if sign else 0
        carries.append(c)
    return carries


def statement(op, x, y):
    """res of a live operation, as include/bpg.h states it: the division of the magnitudes, the sign put back"""
    ax, ay = magnitude(x), magnitude(y)
    if ay == 0:
        return 0
    if op == SDIV:
        return -(ax // ay) & M256 if (x >> 255) != (y >> 255) else ax // ay
    assert op == SMOD
    return -(ax % ay) & M256 if x >> 255 else ax % ay


def honest(op, x, y, exposed):
    """The witness the statement asks for.  A padding row (op neither SDIV nor SMOD) ignores x, y and exposed."""
    is_sdiv, is_smod = int(op == SDIV), int(op == SMOD)
    if not (is_sdiv or is_smod):
        x = y = exposed = 0
    ax, ay = magnitude(x), magnitude(y)
    q, r = divmod(ax, ay) if ay else (0, ax)
    w = {"is_sdiv": is_sdiv, "is_smod": is_smod, "g": int(bool(exposed)), "z": int(y == 0),
         "xl": limbs(x), "yl": limbs(y), "ql": limbs(q), "ayl": limbs(ay),        # limb columns that are not derived
         "xb": x, "yb": y, "axb": ax, "ayb": ay, "qb": q, "rb": r, "db": ay - r - 1 if ay else 0,   # the words the bit columns spell
         "fixed": set()}                                                          # what a forgery states itself: chains() leaves it alone
    chains(w)
    assert word(w["resl"]) == w["resb"] == (statement(op, x, y) if op in LIVE else 0), (op, hex(x), hex(y))
    return w


def chains(w):
    """(Re)derives what follows from the rest of the witness, in the order the constraints tie it: the sign neg, the
    magnitude m, the result, the carries of the product columns, the carry bits of r + d + 1 and of the three negations,
    the inverse of the zero test -- each unless the forgery has fixed it.  A forged witness stays consistent wherever it
    can."""
    fixed = w["fixed"]
    sx, sy = w["xb"] >> 255, w["yb"] >> 255
    rl = limbs(w["rb"])
    if "neg" not in fixed:
        w["neg"] = w["is_sdiv"] * (sx ^ sy) + w["is_smod"] * sx
    if "ml" not in fixed:
        w["ml"] = [(1 - w["z"]) * (w["is_sdiv"] * w["ql"][k] + w["is_smod"] * rl[k]) for k in range(16)]
    if "resb" not in fixed:
        m = word(w["ml"])
        w["resb"] = -m & M256 if w["neg"] else m
    if "resl" not in fixed:
        w["resl"] = limbs(w["resb"])
    if "carry" not in fixed:
        axl = limbs(w["axb"])
        carry, c = [], 0
        for k in range(15):
            total = sum(w["ql"][i] * w["ayl"][k - i] for i in range(k + 1)) + rl[k] + c - axl[k]
            assert total < 1 << 38
            c = (total >> 16) % (1 << CARRY_BITS)
            carry.append(c)
        w["carry"] = carry
    w.update(base.remainder_chain(w, w["yl"]))
    if "cx" not in fixed:
        w["cx"] = negation_chain(sx, limbs(w["xb"]), limbs(w["axb"]))
    w["cy"] = negation_chain(sy, limbs(w["yb"]), limbs(w["ayb"]))
    w["cres"] = negation_chain(w["neg"], w["ml"], limbs(w["resb"]))
    return w


def cells(w):
    """the 2499 cells of the row, as Python integers below p"""
    row = [0] * N_COLS
    row[IS_SDIV], row[IS_SMOD], row[G], row[Z], row[INV], row[NEG] = w["is_sdiv"], w["is_smod"], w["g"], w["z"], w["inv"], w["neg"]
    for k in range(16):
        row[X + k], row[Y + k], row[RES + k], row[Q + k], row[AY + k], row[M + k] = (w["xl"][k], w["yl"][k], w["resl"][k], w["ql"][k],
                                                                                    w["ayl"][k], w["ml"][k])
        row[BORROW + k], row[X_CHAIN + k], row[Y_CHAIN + k], row[RES_CHAIN + k] = w["borrow"][k], w["cx"][k], w["cy"][k], w["cres"][k]
    blocks = ((X_BITS, "xb", 256), (Y_BITS, "yb", 256), (RES_BITS, "resb", 256), (AX_BITS, "axb", 256), (AY_BITS, "ayb", 256),
              (Q_BITS, "qb", 256), (R_BITS, "rb", 256), (D_BITS, "db", 256))
    return base.put_blocks(row, w, blocks, CARRY, CARRY_BITS)


def trace_of(ops):
    """[2499, len(ops)] uint64: the model trace of a list of (op, x, y, exposed)"""
    return base.trace_of(honest, cells, ops)


# ---------------------------------------------------------------------------------------------- the edge list
MIN = 1 << 255                   # the word of -2^255
MAXP = (1 << 255) - 1
HALF = (1 << 128) - 1
# |X| = (2^127 - 1)(2^128 - 1) + 2^128 - 2 over 2^128 - 1: q = 2^127 - 1, r = ay - 1; carry 0x77FF8 out of column 7, the
# largest a search found (19 bits)
EXTREME = ((1 << 127) - 1) * HALF + HALF - 1
LARGEST_CARRY = 0x77FF8
n_ = to_word
EDGE_PAIRS = [(MIN, n_(-1)), (MIN, 1),                                           # the quotient 2^255 that has no positive word; -2^255 itself
              (5, 0), (n_(-7), 0),                                               # y = 0
              (n_(-7), 2), (7, n_(-2)), (n_(-7), n_(-2)),                        # truncation, and whose sign the remainder has
              (n_(-8), 2),                                                       # remainder 0 under sx = 1: -0 = 0
              (n_(-1), MIN),                                                     # |x| < |y| at the largest magnitude
              (EXTREME, HALF), (n_(-EXTREME), HALF),                             # the largest carry, under both signs
              (0, 7), (1, n_(-7)), (2, 1), (MAXP, 2), (n_(1 - MIN), MAXP), (MAXP, n_(1 - MIN)),
              (HALF, n_(-HALF)), (n_(-HALF), 1 << 128), (1 << 128, n_(-(1 << 128))), (n_(-(1 << 128)), HALF),
              (MIN, MIN), (n_(-2), n_(-1))]
PADDING = [(NONE, MIN, 3, 1), (3, 1 << 200 | 5, M256, 1), (0xFF, 7, 0, 0), (0x80, M256, M256, 1)]   # operand words to ignore
PADDING_ROWS = (9, 24, 25, 26)   # where edge_ops() has them


def random_ops(n, seed):
    """seeded operations whose magnitudes have every length from 0 to 255 bits, under either sign; a padding row now and
    then"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        values = [to_word(rng.choice((1, -1)) * rng.getrandbits(rng.randint(0, 255))) for _ in range(2)]
        out.append((rng.choice((SDIV, SDIV, SMOD, SMOD, NONE, 3)), *values, rng.randint(0, 1)))
    return out


def edge_ops():
    """2^5 rows: every edge pair once, the flag and the exposed bit taking turns; a padding row at 9, three more after
    the pairs; random operations"""
    ops = [(SDIV if k % 2 == 0 else SMOD, x, y, (k // 2) % 2) for k, (x, y) in enumerate(EDGE_PAIRS)]
    ops = ops[:9] + PADDING[:1] + ops[9:] + PADDING[1:]
    return ops + random_ops(32 - len(ops), 0x5D10)


def edge_ops_full():
    """2^7 rows: every edge pair under both flags, exposed and not; the padding rows; random operations"""
    ops = [(op, x, y, e) for x, y in EDGE_PAIRS for op in LIVE for e in (1, 0)] + PADDING
    return ops + random_ops(128 - len(ops), 0x5D11)


# ---------------------------------------------------------------------------------------------- wrong witnesses
def _fix(w, **stated):
    w.update(stated)
    w["fixed"] |= set(stated)


def _core(w, q, r):
    """the quotient, the remainder and the slack as stated, every limb and bit column of theirs in line"""
    w.update(qb=q, ql=limbs(q), rb=r, db=(w["ayb"] - r - 1) & M256)


def _floor(w):
    """-7 / 2 as the floor -4 with the floor's remainder 1: 4 * 2 + 1 is not 7"""
    assert (w["axb"], w["ayb"]) == (7, 2)
    _core(w, 4, 1)


def _floor_with_the_divisors_sign(w):
    """-7 % 2 = 1 as Python has it: the floor's remainder, and the sign of y instead of x"""
    _floor(w)
    _fix(w, neg=w["yb"] >> 255)


def _sign_dropped(w):
    """res = q where it is -q"""
    assert w["neg"] == 1 and w["qb"]
    _fix(w, resb=w["qb"])


def _last_carry_cleared(w):
    """res = 2^256 - m as it should be, the chain's last carry bit 0 as if res were m"""
    assert w["neg"] == 1 and word(w["ml"])
    w["poke"] = {RES_CHAIN + 15: 0}


def _magnitude_not_taken(w):
    """ax = x on a negative x, divided as such"""
    assert w["xb"] >> 255
    w.update(axb=w["xb"])
    _core(w, *divmod(w["xb"], w["ayb"]))


def _limb_out_of_range(w):
    """the first carry bit of x + ax cleared: limb 0 of ax becomes ax_0 - 2^16, a negative field element, and limb 1 one
    more -- the same integer ax, so the product columns follow with one more out of column 0.  Only the bits of ax, which
    cannot spell it, stand in the way: bit 15 of limb 0 holds its bit less 2"""
    ax = w["axb"]
    assert w["xb"] >> 255 and w["cx"][0] == 1 and (ax >> 16) & 0xFFFF < 0xFFFF
    _fix(w, cx=[0] + w["cx"][1:], carry=[w["carry"][0] + 1] + w["carry"][1:])
    w.update(axb=ax + B)
    w["poke"] = {AX_BITS + 15: ((ax >> 15) & 1) - 2}


def _big_remainder(w):
    """(q - 1, r + ay) with r = 0: q ay + r = ax still holds, but r = ay; the slack wraps"""
    assert w["rb"] == 0 and w["qb"]
    _core(w, w["qb"] - 1, w["ayb"])


def _wrapped_quotient(w):
    """(q + 1, r - ay), the remainder's limbs wrapped: q' ay + r' = ax + 2^256, r' + d' + 1 = ay + 2^256"""
    _core(w, w["qb"] + 1, (w["rb"] - w["ayb"]) & M256)


def _wrap_high(w):
    """q = ay = 2^128 with x = 0: q ay = 2^256 lies entirely in column 16"""
    assert w["xb"] == 0 and w["ayb"] == 1 << 128
    _core(w, 1 << 128, 0)


def _zero_flag_on_nonzero(w):
    assert w["yb"]
    w.update(z=1)


def _no_zero_flag_on_zero(w):
    """z = 0 on y = 0, the slack wrapped so that every limb of r + d + 1 = ay adds up: the carry out remains"""
    assert w["yb"] == 0
    w.update(z=0, db=(-w["rb"] - 1) & M256)


def _result_on_zero(w):
    assert w["yb"] == 0 and w["xb"]
    _fix(w, resb=w["xb"])


def _neg_flipped(w):
    _fix(w, neg=1 - w["neg"])


def _both_flags(w):
    """SDIV and SMOD at once, g = 0, m = q + r limb by limb: only the flag pair is wrong"""
    assert not (w["xb"] >> 255 or w["yb"] >> 255)
    w.update(is_sdiv=1, is_smod=1, g=0)


def _exposed_padding(w):
    w.update(g=1)


def _flag_no_bit(w):
    """is_sdiv = 2 on positive operands: neg = 0 and m = 2 q, a result that follows"""
    assert not (w["xb"] >> 255 or w["yb"] >> 255)
    w.update(is_sdiv=2, g=0)


def _fat_limb(w):
    """limb column q_0 holds q_0 + 2^16 and q_1 one less: the same integer q, so every product column still adds up
    (under SMOD, where m does not read q)"""
    ql = list(w["ql"])
    assert ql[1] > 0 and w["is_smod"]
    ql[0], ql[1] = ql[0] + B, ql[1] - 1
    w.update(ql=ql, qb=w["qb"] - B)   # the bits spell (q_0, q_1 - 1, ...): only limb 0 differs from its column


def _remainder_as_quotient(w):
    """m = r under SDIV, the result following it"""
    assert w["is_sdiv"] and w["rb"] != w["qb"]
    _fix(w, ml=limbs(w["rb"]))


def _slack_off_by_one(w):
    assert w["db"] & 0xFFFF < 0xFFFF
    w.update(db=w["db"] + 1)


def _non_bit(col, key=None, shift=0):
    def forge(w):
        """bits (1, 0) of a value that is 2 there, written as (0, 2): the same value"""
        assert key is None or (w[key] >> shift) & 3 == 2, (key, hex(w[key]))
        w["poke"] = {col: 2, col + 1: 0}
    return forge


def _free_bit(col, free):
    def forge(w):
        """a carry bit no equation reads on this row -- r + d + 1 under z, a negation that is not taken -- set to 2"""
        assert free(w)
        w["poke"] = {col: 2}
    return forge


def _carry_non_bit(w):
    """4 * 0x8000 + 5 over 0x8000: the carry out of column 0 is 2"""
    assert w["carry"][0] == 2
    w["poke"] = {CARRY: 2, CARRY + 1: 0}


_NEG_POS = (n_(-(0xFEDC << 230 | 0x13579BDF << 90 | 0x246A)), 0xA5A5 << 100 | 0x4242 << 16 | 0x1236)   # q has 9 limbs, r < ay
_POS_NEG = (0xFEDC << 230 | 0x13579BDF << 90 | 0x246A, n_(-(0xA5A5 << 100 | 0x4242 << 16 | 0x1236)))
_SEVEN = (n_(-7), 2)
# (name, the honest operation, the forgery, the families that break -- nothing else may)
CATALOGUE = [("floor_for_truncation", (SDIV,) + _SEVEN + (1,), _floor, {"product"}),
             ("remainder_with_the_divisors_sign", (SMOD,) + _SEVEN + (1,), _floor_with_the_divisors_sign, {"product", "neg"}),
             ("result_with_the_sign_dropped", (SDIV,) + _SEVEN + (1,), _sign_dropped, {"result"}),
             ("negated_result_with_the_last_carry_cleared", (SDIV,) + _NEG_POS + (1,), _last_carry_cleared, {"result"}),
             ("magnitude_not_taken", (SDIV,) + _NEG_POS + (1,), _magnitude_not_taken, {"magnitude"}),
             ("magnitude_limb_out_of_range", (SMOD,) + _NEG_POS + (0,), _limb_out_of_range, {"magnitude_bits"}),
             ("remainder_equal_to_the_divisor", (SDIV, n_(-8), 2, 1), _big_remainder, {"remainder_top"}),
             ("wrapped_quotient", (SDIV,) + _NEG_POS + (1,), _wrapped_quotient, {"product", "remainder_top"}),
             ("wrap_in_the_high_columns", (SDIV, 0, n_(-(1 << 128)), 1), _wrap_high, {"high"}),
             ("zero_flag_on_y_not_zero", (SMOD,) + _POS_NEG + (0,), _zero_flag_on_nonzero, {"zero"}),
             ("no_zero_flag_on_y_zero", (SDIV, n_(-7), 0, 1), _no_zero_flag_on_zero, {"zero", "remainder_top"}),
             ("result_on_y_zero", (SDIV, 0x77 << 200 | 5, 0, 1), _result_on_zero, {"result"}),
             ("neg_flipped", (SDIV,) + _SEVEN + (1,), _neg_flipped, {"neg"}),
             ("both_flags", (SDIV, 7, 2, 0), _both_flags, {"one_flag"}),
             ("exposed_padding_row", (NONE, 0, 0, 0), _exposed_padding, {"filter"}),
             ("flag_that_is_no_bit", (SDIV, 7, 2, 0), _flag_no_bit, {"flags"}),
             ("limb_of_two_to_the_16", (SMOD,) + _NEG_POS + (1,), _fat_limb, {"limbs"}),
             ("remainder_as_quotient", (SDIV,) + _POS_NEG + (1,), _remainder_as_quotient, {"m"}),
             ("slack_off_by_one", (SMOD,) + _POS_NEG + (1,), _slack_off_by_one, {"remainder"}),
             ("non_bit_in_x", (SDIV, 2, 1, 1), _non_bit(X_BITS, "xb"), {"operand_bits"}),
             ("non_bit_in_y", (SDIV, 7, 2, 1), _non_bit(Y_BITS, "yb"), {"operand_bits"}),
             ("non_bit_in_res", (SDIV, 2, 1, 1), _non_bit(RES_BITS, "resb"), {"operand_bits"}),
             ("non_bit_in_ax", (SDIV, n_(-2), 1, 1), _non_bit(AX_BITS, "axb"), {"magnitude_bits"}),
             ("non_bit_in_ay", (SDIV, 7, n_(-2), 1), _non_bit(AY_BITS, "ayb"), {"magnitude_bits"}),
             ("non_bit_in_q", (SMOD, 5, 2, 1), _non_bit(Q_BITS, "qb"), {"core_bits"}),
             ("non_bit_in_r", (SMOD, n_(-2), 7, 1), _non_bit(R_BITS, "rb"), {"core_bits"}),
             ("non_bit_in_d", (SMOD, 7 * (1 << 40) + 5, (1 << 40) | 0x20000 | 8, 1), _non_bit(D_BITS + 16, "db", 16), {"core_bits"}),
             ("non_bit_in_a_carry", (SDIV, n_(-0x20005), 0x8000, 0), _carry_non_bit, {"carry_bits"}),
             ("non_bit_in_the_remainders_carry", (SDIV, 5, 0, 1), _free_bit(BORROW + 3, lambda w: w["z"]), {"borrow_bits"}),
             ("non_bit_in_the_carry_of_x", (SDIV, 7, n_(-2), 1), _free_bit(X_CHAIN + 3, lambda w: 1 - (w["xb"] >> 255)), {"chain_bits"}),
             ("non_bit_in_the_carry_of_y", (SDIV, n_(-7), 2, 1), _free_bit(Y_CHAIN + 3, lambda w: 1 - (w["yb"] >> 255)), {"chain_bits"}),
             ("non_bit_in_the_carry_of_res", (SDIV, 7, 2, 1), _free_bit(RES_CHAIN + 15, lambda w: 1 - w["neg"]), {"chain_bits"})]


def forged(entry):
    """the cells of a catalogue entry's row"""
    return base.forged(honest, chains, cells, entry)


def family_of(index):
    return base.family_of(FAMILIES, index)
