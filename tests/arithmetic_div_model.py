"""An independent model of the division table (proof_protocol_decoder_amd/arithmetic_div.py, csrc/arithmetic_div.hip),
shared by tests/test_arithmetic_div.py and tests/test_gpu_arithmetic_div.py.  It works from the statement in
include/bpg.h and the column list in AIRS.md section 2 ("Division (a shipped program)") over Python integers (divmod):
it imports nothing of the package, so the column map below is a third statement of it and the tests compare it with the
package's.  What it shares with the modular table's model is in tests/word_table_model.py, as independent as this file.

    w = honest(op, x, y, exposed)     the witness of one operation: a dict of what a row holds
    cells(w)                          the 1650 cells of its row
    CATALOGUE                         wrong witnesses, each otherwise consistent: (name, operation, forge, families broken)
"""
import word_table_model as base
from word_table_model import B, M256, P, limbs, word  # noqa: F401 (the tests read them here)

NONE, DIV, MOD = 0, 1, 2
LIVE = (DIV, MOD)
CARRY_BITS = 19

# AIRS.md section 2: five single columns, four limb blocks, five bit blocks, 15 carries of 19 bits, 16 carry bits of r + d + 1
IS_DIV, IS_MOD, G, Z, INV = range(5)
X, Y, RES, Q = 5, 21, 37, 53
X_BITS, Y_BITS, Q_BITS, R_BITS, D_BITS = 69, 325, 581, 837, 1093
CARRY, BORROW, N_COLS = 1349, 1634, 1650
# the families in constraint order, with their sizes
FAMILIES = [("flags", 3), ("one_flag", 1), ("filter", 1), ("zero", 2), ("high", 1), ("x_bits", 256), ("y_bits", 256),
            ("q_bits", 256), ("r_bits", 256), ("d_bits", 256), ("carry_bits", 285), ("borrow_bits", 16), ("x_limbs", 16),
            ("y_limbs", 16), ("q_limbs", 16), ("product", 16), ("remainder", 16), ("remainder_top", 1), ("result", 16)]
N_CONSTRAINTS = sum(c for _, c in FAMILIES)   # 1686


def honest(op, x, y, exposed):
    """The witness the statement asks for.  A padding row (op neither DIV nor MOD) ignores x, y and exposed."""
    is_div, is_mod = int(op == DIV), int(op == MOD)
    if not (is_div or is_mod):
        x = y = exposed = 0
    q, r = divmod(x, y) if y else (0, x)
    res = 0 if y == 0 else q if is_div else r
    w = {"is_div": is_div, "is_mod": is_mod, "g": int(bool(exposed)), "z": int(y == 0),
         "xl": limbs(x), "yl": limbs(y), "ql": limbs(q), "resl": limbs(res),     # the limb columns
         "xb": x, "yb": y, "qb": q, "rb": r, "db": y - r - 1 if y else 0}         # the words the bit columns spell
    return chains(w)


def chains(w):
    """(Re)derives what follows from the rest of the witness: the carries of the product columns, the carry bits of
    r + d + 1, and the inverse of the zero test.  A forged witness stays consistent wherever it can."""
    xb, rb = limbs(w["xb"]), limbs(w["rb"])
    carry, c = [], 0
    for k in range(15):
        total = sum(w["ql"][i] * w["yl"][k - i] for i in range(k + 1)) + rb[k] + c - xb[k]
        assert total < 1 << 38
        c = (total >> 16) % (1 << CARRY_BITS)
        carry.append(c)
    w.update(carry=carry, **base.remainder_chain(w, w["yl"]))
    return w


def cells(w):
    """the 1650 cells of the row, as Python integers below p"""
    row = [0] * N_COLS
    row[IS_DIV], row[IS_MOD], row[G], row[Z], row[INV] = w["is_div"], w["is_mod"], w["g"], w["z"], w["inv"]
    for k in range(16):
        row[X + k], row[Y + k], row[RES + k], row[Q + k] = w["xl"][k], w["yl"][k], w["resl"][k], w["ql"][k]
        row[BORROW + k] = w["borrow"][k]
    blocks = ((X_BITS, "xb", 256), (Y_BITS, "yb", 256), (Q_BITS, "qb", 256), (R_BITS, "rb", 256), (D_BITS, "db", 256))
    return base.put_blocks(row, w, blocks, CARRY, CARRY_BITS)


def trace_of(ops):
    """[1650, len(ops)] uint64: the model trace of a list of (op, x, y, exposed)"""
    return base.trace_of(honest, cells, ops)


# ---------------------------------------------------------------------------------------------- the edge list
MAX = M256
HALF = (1 << 128) - 1
# q = y = 2^128 - 1, r = y - 1: eight products of 0xFFFF * 0xFFFF in column 7, carry 0x7FFF7 out of it (19 bits)
LARGEST_CARRY = (HALF * HALF + HALF - 1, HALF)
EDGE_PAIRS = [(0, 0), (0x1234 << 200 | 77, 0),                                   # y = 0
              (0xDEADBEEF << 190 | 0xC0FFEE, 1),                                 # y = 1
              (0, 0xABCD << 100 | 9),                                            # x = 0
              (0x5555 << 64, 0x5555 << 64 | 1 << 250),                           # x < y
              (0x9876 << 240 | 0x1111 << 16, 0x9876 << 240 | 0x1111 << 16),      # x = y
              ((0x4321 << 128) - 1, 0x4321 << 128),                              # x = y - 1
              (MAX, MAX), (MAX, 2), (MAX, HALF), (MAX, 1 << 128), (MAX, 1 << 255),
              (MAX - 12345, 0x8001 << 240),                                      # y: only the top limb
              (0xFEDCBA9876543210 << 150 | 0xFFFF, 0xFFFE),                      # y: only the bottom limb
              (5 * (0x7777 << 80 | 3) + (0x7777 << 80 | 3) - 1, 0x7777 << 80 | 3),  # r = y - 1: slack zero
              (5 * (0x7777 << 80 | 3), 0x7777 << 80 | 3),                        # r = 0: slack y - 1
              (0xFFFF << (16 * 9), 0xFFFF << (16 * 3)),                          # one limb of 0xFFFF each
              LARGEST_CARRY]
PADDING = [(NONE, MAX, 3, 1), (3, 1 << 200 | 5, MAX, 1), (0xFF, 7, 0, 0), (0x80, MAX, MAX, 1)]   # operand words to ignore


def random_ops(n, seed):
    """seeded operations whose operands have every length from 0 to 256 bits, a padding row now and then"""
    return base.random_ops(n, seed, 2, (DIV, DIV, MOD, MOD, NONE, 3))


def edge_ops():
    """2^5 rows: every edge pair once, the flag and the exposed bit taking turns; the padding rows; random operations"""
    ops = [(DIV if k % 2 == 0 else MOD, x, y, (k // 2) % 2) for k, (x, y) in enumerate(EDGE_PAIRS)] + PADDING
    return ops + random_ops(32 - len(ops), 0xD1F0)


def edge_ops_full():
    """2^7 rows: every edge pair under both flags, exposed and not; the padding rows; random operations"""
    ops = [(op, x, y, e) for x, y in EDGE_PAIRS for op in (DIV, MOD) for e in (1, 0)] + PADDING
    return ops + random_ops(128 - len(ops), 0xD1F1)


# ---------------------------------------------------------------------------------------------- wrong witnesses
def _wrapped_quotient(w):
    """(q + 1, r - y), the remainder's limbs wrapped: q' y + r' = x + 2^256, r' + d' + 1 = y + 2^256"""
    q, r, y = w["qb"] + 1, (w["rb"] - w["yb"]) & M256, w["yb"]
    w.update(qb=q, ql=limbs(q), resl=limbs(q), rb=r, db=(y - r - 1) & M256)


def _big_remainder(w):
    """(q - 1, r + y): q y + r = x still holds, but r >= y; the slack wraps"""
    q, r, y = w["qb"] - 1, w["rb"] + w["yb"], w["yb"]
    assert q >= 0 and r <= M256
    w.update(qb=q, ql=limbs(q), resl=limbs(q), rb=r, db=(y - r - 1) & M256)


def _wrap_high(w):
    """q = y = 2^128 with x = 0: q y = 2^256 lies entirely in column 16"""
    q = 1 << 128
    w.update(qb=q, ql=limbs(q), resl=limbs(q), rb=0, db=w["yb"] - 1)


def _wrap_carry(w):
    """q = 2^255, y = 2 with x = 0: column 15 holds 2^16, a carry the table has no column for"""
    q = 1 << 255
    w.update(qb=q, ql=limbs(q), resl=limbs(q), rb=0, db=w["yb"] - 1)


def _result_on_zero(w):
    w.update(resl=limbs(w["xb"]))


def _zero_flag_on_nonzero(w):
    w.update(z=1, resl=limbs(0))


def _mod_under_div(w):
    w.update(resl=limbs(w["rb"]))


def _both_flags(w):
    w.update(is_div=1, is_mod=1, g=0, resl=[a + b for a, b in zip(w["ql"], limbs(w["rb"]))])


def _fat_limb(w):
    """limb column q_0 holds q_0 + 2^16 and q_1 one less: the same integer q, so every product column still adds up"""
    ql = list(w["ql"])
    assert ql[1] > 0
    ql[0], ql[1] = ql[0] + B, ql[1] - 1
    w.update(ql=ql, resl=list(ql), qb=w["qb"] - B)   # the bits spell (q_0, q_1 - 1, ...): only limb 0 differs from its column


def _non_bit(w):
    """bits 1, 0 of the slack (value 2) written as 0, 2: the limb's sum is unchanged"""
    assert (w["db"] >> 16) & 3 == 2
    w["poke"] = {D_BITS + 16: 2, D_BITS + 17: 0}


def _exposed_padding(w):
    w.update(g=1)


_XY = (0xFEDC << 230 | 0x13579BDF << 90 | 0x2468, 0xA5A5 << 100 | 0x4242 << 16 | 0x1235)   # q has 9 limbs, r < y
# (name, the honest operation, the forgery, the families that break -- nothing else may)
CATALOGUE = [("wrapped_quotient", (DIV,) + _XY + (1,), _wrapped_quotient, {"product", "remainder_top"}),
             ("remainder_not_below_y", (DIV,) + _XY + (1,), _big_remainder, {"remainder_top"}),
             ("wrap_in_the_high_columns", (DIV, 0, 1 << 128, 1), _wrap_high, {"high"}),
             ("wrap_out_of_column_15", (DIV, 0, 2, 0), _wrap_carry, {"product"}),
             ("result_on_y_zero", (DIV, 0x77 << 200 | 5, 0, 1), _result_on_zero, {"result"}),
             ("zero_flag_on_y_not_zero", (MOD,) + _XY + (0,), _zero_flag_on_nonzero, {"zero"}),
             ("remainder_as_quotient", (DIV,) + _XY + (1,), _mod_under_div, {"result"}),
             ("both_flags", (DIV,) + _XY + (1,), _both_flags, {"one_flag"}),
             ("limb_of_two_to_the_16", (DIV,) + _XY + (1,), _fat_limb, {"q_limbs"}),
             ("non_bit", (MOD, 7 * (1 << 40) + 5, (1 << 40) | 0x20000 | 8, 1), _non_bit, {"d_bits"}),
             ("exposed_padding_row", (NONE, 0, 0, 0), _exposed_padding, {"filter"})]


def forged(entry):
    """the cells of a catalogue entry's row"""
    return base.forged(honest, chains, cells, entry)


def family_of(index):
    return base.family_of(FAMILIES, index)
