"""An independent model of the modular table (proof_protocol_decoder_amd/arithmetic_mod.py, csrc/arithmetic_mod.hip),
shared by tests/test_arithmetic_mod.py and tests/test_gpu_arithmetic_mod.py.  It works from the statement in
include/bpg.h and the column list in AIRS.md section 2 ("Modular (a shipped program)") over Python integers (divmod, %):
it imports nothing of the package, so the column map below is a third statement of it and the tests compare it with the
package's.  What it shares with the division table's model is in tests/word_table_model.py, as independent as this file.

    w = honest(op, a, b, m, exposed)  the witness of one operation: a dict of what a row holds
    cells(w)                          the 2560 cells of its row
    CATALOGUE                         wrong witnesses, each otherwise consistent: (name, operation, forge, families broken)
"""
import word_table_model as base
from word_table_model import B, M256, P, limbs, word  # noqa: F401 (the tests read them here)

NONE, ADDMOD, MULMOD = 0, 1, 2
LIVE = (ADDMOD, MULMOD)
CARRY_BITS, CARRY_OFFSET = 21, 1 << 20

# AIRS.md section 2: five single columns, four blocks of 16 limbs and one of 32, six bit blocks, 31 carries of 21 bits, 16
# carry bits of r + d + 1
IS_ADDMOD, IS_MULMOD, G, Z, INV = range(5)
A, B_, M, RES, Q = 5, 21, 37, 53, 69
A_BITS, B_BITS, M_BITS, Q_BITS, R_BITS, D_BITS = 101, 357, 613, 869, 1381, 1637
CARRY, BORROW, N_COLS = 1893, 2544, 2560
# the families in constraint order, with their sizes
FAMILIES = [("flags", 3), ("one_flag", 1), ("filter", 1), ("zero", 2), ("high", 1), ("a_bits", 256), ("b_bits", 256),
            ("m_bits", 256), ("q_bits", 512), ("r_bits", 256), ("d_bits", 256), ("carry_bits", 651), ("borrow_bits", 16),
            ("abm_limbs", 48), ("q_limbs", 32), ("product", 32), ("remainder", 16), ("remainder_top", 1), ("result", 16)]
N_CONSTRAINTS = sum(c for _, c in FAMILIES)   # 2612


def intermediate(is_addmod, is_mulmod, a, b):
    """U over the integers: 257 bits for the sum, 512 for the product, nothing wrapped"""
    return is_addmod * (a + b) + is_mulmod * (a * b)


def honest(op, a, b, m, exposed):
    """The witness the statement asks for.  A padding row (op neither ADDMOD nor MULMOD) ignores a, b, m and exposed."""
    is_addmod, is_mulmod = int(op == ADDMOD), int(op == MULMOD)
    if not (is_addmod or is_mulmod):
        a = b = m = exposed = 0
    u = intermediate(is_addmod, is_mulmod, a, b)
    q, r = divmod(u, m) if m else (u >> 256, u & M256)          # a zero modulus divides as M = 2^256
    res = u % m if m else 0
    w = {"is_addmod": is_addmod, "is_mulmod": is_mulmod, "g": int(bool(exposed)), "z": int(m == 0),
         "al": limbs(a), "bl": limbs(b), "ml": limbs(m), "ql": limbs(q, 32), "resl": limbs(res),   # the limb columns
         "ab": a, "bb": b, "mb": m, "qb": q, "rb": r, "db": m - r - 1 if m else 0}                # the words the bit columns spell
    return chains(w)


def chains(w):
    """(Re)derives what follows from the rest of the witness: the signed carries of the product columns, the carry bits
    of r + d + 1, and the inverse of the zero test.  A forged witness stays consistent wherever it can."""
    rb = limbs(w["rb"])
    big_m = w["ml"] + [w["z"]]                                   # the 17 limbs of M = m + z 2^256
    carry, signed, c = [], [], 0
    for k in range(31):
        left = w["is_mulmod"] * sum(w["al"][i] * w["bl"][k - i] for i in range(16) if 0 <= k - i < 16)
        right = sum(w["ql"][k - j] * big_m[j] for j in range(17) if 0 <= k - j < 32)
        if k < 16:
            left += w["is_addmod"] * (w["al"][k] + w["bl"][k])
            right += rb[k]
        total = left - right + c
        assert abs(total) < 1 << 38
        c = total >> 16                                          # floor: exact on an honest row
        signed.append(c)
        carry.append((c + CARRY_OFFSET) % (1 << CARRY_BITS))
    w.update(carry=carry, signed_carry=signed, **base.remainder_chain(w, w["ml"]))
    return w


def cells(w):
    """the 2560 cells of the row, as Python integers below p"""
    row = [0] * N_COLS
    row[IS_ADDMOD], row[IS_MULMOD], row[G], row[Z], row[INV] = w["is_addmod"], w["is_mulmod"], w["g"], w["z"], w["inv"]
    for k in range(16):
        row[A + k], row[B_ + k], row[M + k], row[RES + k] = w["al"][k], w["bl"][k], w["ml"][k], w["resl"][k]
        row[BORROW + k] = w["borrow"][k]
    for k in range(32):
        row[Q + k] = w["ql"][k]
    blocks = ((A_BITS, "ab", 256), (B_BITS, "bb", 256), (M_BITS, "mb", 256), (Q_BITS, "qb", 512), (R_BITS, "rb", 256),
              (D_BITS, "db", 256))
    return base.put_blocks(row, w, blocks, CARRY, CARRY_BITS)


def trace_of(ops):
    """[2560, len(ops)] uint64: the model trace of a list of (op, a, b, m, exposed)"""
    return base.trace_of(honest, cells, ops)


# ---------------------------------------------------------------------------------------------- the edge list
MAX = M256
G1 = 0xFEDC << 240 | 0x13579BDF2468ACE << 120 | 0x9999 << 16 | 0x7
G2 = 0xC0DE << 240 | 0xFFFF0000FFFF << 96 | 0x1235
MX = 0x7777 << 80 | 3
# the two carries of largest magnitude (AIRS.md): both under MULMOD
MOST_NEGATIVE = (MAX - 1, 1 << 255, MAX)      # -0xEFFF1
MOST_POSITIVE = (MAX, MAX, 0)                 # +0xFFFEF, the multiplication table's largest carry: with m = 0 the right side is small
EDGE_TRIPLES = [MOST_NEGATIVE, MOST_POSITIVE,
                (0, 0, 0), (G1, G2, 0),                                  # m = 0; a + b >= 2^256 there
                (G1, G2, 1), (MAX, MAX, 1),                              # m = 1: r = 0, q = U, 512 bits of it under MULMOD
                (G1, G2, 2), (MAX, MAX, 2),
                (G1, G2, MAX), (MAX, MAX, MAX),
                (MAX, MAX, 3), (MAX, 1, 2),                              # a + b >= 2^256 over a small m: q of 257 bits
                (MX - 1, 0, MX),                                         # ADDMOD: r = m - 1 (slack zero); MULMOD: U = 0
                (MX - 1, 1, MX),                                         # MULMOD: r = m - 1; ADDMOD: r = 0 (slack m - 1)
                (0, 0, MX), (0, G2, MX),                                 # a = b = 0; a = 0
                (0x1234, 0x5678, 1 << 200),                              # U < m: q = 0
                (G1, G2, 0x8001 << 240),                                 # m: only the top limb
                (G1, G2, 0xFFFE),                                        # m: only the bottom limb
                (1 << 255, 2, 1 << 128)]
PADDING = [(NONE, MAX, 3, G1, 1), (3, 1 << 200 | 5, MAX, 0, 1), (0xFF, 7, 0, MAX, 0), (0x80, MAX, MAX, MAX, 1)]   # operand words to ignore


def random_ops(n, seed):
    """seeded operations whose operands have every length from 0 to 256 bits, a padding row now and then"""
    return base.random_ops(n, seed, 3, (ADDMOD, ADDMOD, MULMOD, MULMOD, MULMOD, NONE, 3))


def edge_ops():
    """2^5 rows: every edge triple once -- the two extremes under MULMOD, then ADDMOD at the even places and MULMOD at the
    odd ones, the exposed bit changing every second row --; the padding rows; random operations"""
    ops = [(MULMOD if k < 2 or k % 2 else ADDMOD, a, b, m, (k // 2) % 2) for k, (a, b, m) in enumerate(EDGE_TRIPLES)] + PADDING
    return ops + random_ops(32 - len(ops), 0xA0D0)


def edge_ops_full():
    """2^7 rows: every edge triple under both flags, exposed and not; the padding rows; random operations"""
    ops = [(op, a, b, m, e) for a, b, m in EDGE_TRIPLES for op in (ADDMOD, MULMOD) for e in (1, 0)] + PADDING
    return ops + random_ops(128 - len(ops), 0xA0D1)


# ---------------------------------------------------------------------------------------------- wrong witnesses
def _set_qr(w, q, r):
    """a quotient and a remainder with everything that follows from them: the result and the slack"""
    m = w["mb"]
    w.update(qb=q, ql=limbs(q, 32), rb=r, resl=limbs(0 if w["z"] else r), db=(m - r - 1) & M256 if not w["z"] else 0)


def _reduced_first(w):
    """U taken modulo 2^256 before it is reduced modulo m -- the mistake this table exists for.  q M + r = U - 2^256 t:
    the low sixteen columns add up, the first column above them that sees the missing part does not"""
    u = intermediate(w["is_addmod"], w["is_mulmod"], w["ab"], w["bb"])
    assert u >> 256 and w["mb"]
    _set_qr(w, *divmod(u & M256, w["mb"]))


def _wrap_into_column_31(w):
    """q = 2^257, m = 2^255 with U = 0: q M = 2^512 lies in column 31 as 2^16, a carry the table has no column for"""
    assert (w["ab"], w["bb"], w["mb"]) == (0, 0, 1 << 255)
    _set_qr(w, 1 << 257, 0)


def _wrap_into_the_high_columns(w):
    """q = 2^272, m = 2^240 with U = 0: q M = 2^512 lies entirely in column 32"""
    assert (w["ab"], w["bb"], w["mb"]) == (0, 0, 1 << 240)
    _set_qr(w, 1 << 272, 0)


def _not_reduced(w):
    """(q - 1, r + m): q M + r = U still holds, but r >= m; the slack wraps"""
    q, r = w["qb"] - 1, w["rb"] + w["mb"]
    assert q >= 0 and r <= M256
    _set_qr(w, q, r)


def _zero_flag_on_nonzero(w):
    """z = 1 with m != 0, and everything else in line with it: M = m + 2^256, res = 0"""
    u = intermediate(w["is_addmod"], w["is_mulmod"], w["ab"], w["bb"])
    w.update(z=1)
    _set_qr(w, *divmod(u, w["mb"] + (1 << 256)))


def _no_zero_flag_on_zero(w):
    """z = 0 with m = 0: M = 0, so r = U (which the operands here keep below 2^256); r + d + 1 = 0 only with a carry out"""
    u = intermediate(w["is_addmod"], w["is_mulmod"], w["ab"], w["bb"])
    assert w["mb"] == 0 and u <= M256
    w.update(z=0)
    _set_qr(w, 0, u)


def _result_on_zero(w):
    assert w["mb"] == 0 and w["rb"]
    w.update(resl=limbs(w["rb"]))


def _both_flags(w):
    """both flags, U = a b + a + b (below 2^512) divided honestly: only the flag pair is wrong"""
    w.update(is_addmod=1, is_mulmod=1, g=0)
    _set_qr(w, *divmod(w["ab"] * w["bb"] + w["ab"] + w["bb"], w["mb"]))


def _sum_under_mulmod(w):
    assert w["is_mulmod"]
    _set_qr(w, *divmod(w["ab"] + w["bb"], w["mb"]))


def _exposed_padding(w):
    w.update(g=1)


def _non_bit(w):
    """bits 20, 19 of the first carry column group (c_0 + 2^20 with 0 <= c_0 < 2^19: bits 1, 0) written as 0, 2"""
    assert w["carry"][0] >> 19 == 2
    w["poke"] = {CARRY + 19: 2, CARRY + 20: 0}


def _fat_limb(w):
    """limb column q_0 holds q_0 + 2^16 and q_1 one less: the same integer q, so every product column still adds up"""
    ql = list(w["ql"])
    assert ql[1] > 0
    ql[0], ql[1] = ql[0] + B, ql[1] - 1
    w.update(ql=ql, qb=w["qb"] - B)   # the bits spell (q_0, q_1 - 1, ...): only limb 0 differs from its column


def _quotient_as_result(w):
    assert w["qb"] & M256 != w["rb"]
    w.update(resl=limbs(w["qb"] & M256))


_ABM = (G1, G2, 0xA5A5 << 180 | 0x4242 << 16 | 0x1235)      # a + b >= 2^256; q has 6 limbs (ADDMOD), 21 (MULMOD); r < m
# (name, the honest operation, the forgery, the families that break -- nothing else may)
CATALOGUE = [("addmod_of_the_wrapped_sum", (ADDMOD,) + _ABM + (1,), _reduced_first, {"product"}),
             ("mulmod_of_the_low_half", (MULMOD,) + _ABM + (1,), _reduced_first, {"product"}),
             ("wrap_into_column_31", (ADDMOD, 0, 0, 1 << 255, 0), _wrap_into_column_31, {"product"}),
             ("wrap_into_the_high_columns", (ADDMOD, 0, 0, 1 << 240, 1), _wrap_into_the_high_columns, {"high"}),
             ("result_not_reduced", (MULMOD,) + _ABM + (1,), _not_reduced, {"remainder_top"}),
             ("zero_flag_on_m_not_zero", (MULMOD,) + _ABM + (0,), _zero_flag_on_nonzero, {"zero"}),
             ("no_zero_flag_on_m_zero", (ADDMOD, 0x77 << 200 | 5, 0x1234, 0, 1), _no_zero_flag_on_zero, {"zero", "remainder_top"}),
             ("result_on_m_zero", (ADDMOD, 0x77 << 200 | 5, 0x1234, 0, 1), _result_on_zero, {"result"}),
             ("both_flags", (MULMOD,) + _ABM + (1,), _both_flags, {"one_flag"}),
             ("sum_under_mulmod", (MULMOD,) + _ABM + (1,), _sum_under_mulmod, {"product"}),
             ("exposed_padding_row", (NONE, 0, 0, 0, 0), _exposed_padding, {"filter"}),
             ("non_bit_in_a_carry", (ADDMOD, 5, 6, 7, 1), _non_bit, {"carry_bits"}),
             ("limb_of_two_to_the_16", (MULMOD,) + _ABM + (1,), _fat_limb, {"q_limbs"}),
             ("quotient_as_result", (MULMOD,) + _ABM + (1,), _quotient_as_result, {"result"})]


def forged(entry):
    """the cells of a catalogue entry's row"""
    return base.forged(honest, chains, cells, entry)


def family_of(index):
    return base.family_of(FAMILIES, index)
