"""Integer model of the radix-16 passes of the 2^12..2^14-point NTT block kernels (csrc/ntt.hip, dit16 / dif16): one
twiddle layer plus a 16-point DFT whose twiddles are powers of two must equal the four table-twiddle radix-2 stages they
replace, and the limb arithmetic of gl::mul_pow2 (csrc/gl.hpp) must equal multiplication by 2^S mod p.  Python integers
only: no GPU, no library."""
import random

import pytest

P = (1 << 64) - (1 << 32) + 1
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
TWO_ADIC_ROOT = 1753635133440165772  # 7^((p-1)/2^32), gl.hpp


def root(k):
    r = TWO_ADIC_ROOT
    for _ in range(k, 32):
        r = r * r % P
    return r


def brev4(m):
    return ((m & 1) << 3) | ((m & 2) << 1) | ((m & 4) >> 1) | ((m & 8) >> 3)


def test_powers_of_the_16th_root_are_signed_powers_of_two():
    w = root(4)
    assert w == pow(2, 156, P) == P - (1 << 60) and pow(w, 16, P) == 1 and pow(w, 8, P) == P - 1
    assert root(3) == pow(2, 120, P) == P - (1 << 24) and root(2) == 1 << 48
    assert pow(2, 96, P) == P - 1
    signed = {pow(2, 12 * k, P): "+%d" % k for k in range(8)}
    signed.update({P - pow(2, 12 * k, P): "-%d" % k for k in range(8)})
    for w16 in (w, pow(w, P - 2, P)):
        powers = [pow(w16, e, P) for e in range(16)]
        assert all(v in signed for v in powers) and len(set(powers)) == 16
    # the DFT the kernels run uses the 16th root g = 2^12 itself, whose powers below the 8th carry no sign; the forward
    # root is g^13 and the inverse one g^3, which only permutes the DFT's outputs (dit16 / dif16 below)
    g = 1 << 12
    assert pow(g, 16, P) == 1 and pow(g, 8, P) == P - 1 and pow(g, 13, P) == w and pow(g, 3, P) == pow(w, P - 2, P)


# ---- gl::mul_pow2: the device's limb steps, carry for carry
def shl96(x, s):
    x0, x1 = x & M32, x >> 32
    return (x0 << s) & M32, ((x1 << s) | (x0 >> (32 - s))) & M32, x1 >> (32 - s)


def plus_eps(v, carry):     # x + m*EPS as (lo - m) + (hi + (m & ~borrow)) * 2^32: may not wrap
    if not carry:
        return v
    lo, hi = v & M32, v >> 32
    b = lo == 0
    lo = (lo - 1) & M32
    hi = hi + (0 if b else 1)
    assert hi <= M32, "the +EPS correction wrapped"
    return (hi << 32) | lo


def minus_eps(v, borrow):   # x - m*EPS as (lo + m) + (hi - (m & ~carry)) * 2^32: may not borrow
    if not borrow:
        return v
    lo, hi = v & M32, v >> 32
    c = lo == M32
    lo = (lo + 1) & M32
    hi = hi - (0 if c else 1)
    assert hi >= 0, "the -EPS correction borrowed"
    return (hi << 32) | lo


def mul_pow2_lo(x, s):
    l0, l1, l2 = shl96(x, s)
    v = ((l1 << 32) | l0) + l2 * M32
    return plus_eps(v & M64, v >> 64)


def mul_2p32(y):
    v = (y >> 32) * M32
    assert v <= M64
    hi = (v >> 32) + (y & M32)
    return plus_eps(((hi & M32) << 32) | (v & M32), hi >> 32)


def mul_pow2_hi(x, s):
    l0, l1, l2 = shl96(x, s)
    d = l0 * M32 - ((l2 << 32) | l1)
    return minus_eps(d & M64, d < 0)


def mul_pow2(x, S):
    if S < 32:
        return mul_pow2_lo(x, S)
    if S < 64:
        return mul_2p32(mul_pow2_lo(x, S - 32))
    return mul_pow2_hi(x, S - 64)


def mul_pow2_portable(x, S):  # the host form: reduce128 of the shifted value
    def reduce128(lo, hi):
        hh, hl = hi >> 32, hi & M32
        t0 = (lo - hh) & M64
        if lo < hh:
            t0 = (t0 - M32) & M64
        t1 = ((hl << 32) - hl) & M64
        r = (t0 + t1) & M64
        return (r + M32) & M64 if r < t1 else r
    if S < 64:
        return reduce128((x << S) & M64, x >> (64 - S))
    s = S - 64
    lo, hi = (x << s) & M64, x >> (64 - s)
    a, b = reduce128(0, lo), hi << 32
    d = (a - b) & M64
    return (d - M32) & M64 if a < b else d


EDGE = [0, 1, 2, 7, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, P - 1, P, P + 1, (1 << 63), (1 << 64) - 1,
        (1 << 64) - (1 << 32), (1 << 64) - (1 << 32) - 1, 0xFFFFFFFF00000000, 0x00000000FFFFFFFF,
        0xFFFFFFFEFFFFFFFF, 0x8000000080000000, P - (1 << 32), (1 << 48) + 12345]


def test_mul_pow2_limb_steps_equal_multiplication_by_a_power_of_two():
    rng = random.Random(5)
    xs = EDGE + [rng.getrandbits(64) for _ in range(4096)]
    # words whose shifted limbs are all ones / all zeros, for every shift: the carry and borrow edges
    for k in range(1, 8):
        s = 12 * k % 32
        xs += [M64 >> s, (M64 >> s) + 1, ((1 << (32 - s)) - 1) << 32, (1 << (64 - s)) - 1, M32 >> s, (M32 >> s) << 32 | M32]
    for k in range(1, 8):
        S = 12 * k
        for x in xs:
            want = (x << S) % P
            got = mul_pow2(x, S)
            assert 0 <= got <= M64 and got % P == want, (k, hex(x))
            got = mul_pow2_portable(x, S)
            assert 0 <= got <= M64 and got % P == want, ("portable", k, hex(x))


# ---- the passes
def radix2_stages_dit(x, w_s, j, sub):
    """dit_butterflies<4>: x[m] at position j + m*sub of a block of S = 16 sub; twiddles from the table of w_s = w_S"""
    x = list(x)
    for s in range(4):
        step = 1 << s
        for m in range(16):
            if m & step:
                continue
            p = j + (m & (step - 1)) * sub
            t = x[m + step] * pow(w_s, p << (3 - s), P) % P
            x[m], x[m + step] = (x[m] + t) % P, (x[m] - t) % P
    return x


def radix2_stages_dif(x, w_s, j, sub):
    x = list(x)
    for s in range(4):
        half = 8 >> s
        for m in range(16):
            if m & half:
                continue
            p = j + (m & (half - 1)) * sub
            a, b = x[m], x[m + half]
            x[m], x[m + half] = (a + b) % P, (a - b) * pow(w_s, p << s, P) % P
    return x


def pow2_targets(s, dif):
    """(register, exponent S) of stage s: pow2_plan of ntt.hip"""
    out = []
    for k in range(8):
        h = (8 >> s) if dif else (1 << s)
        m = (k // h) * 2 * h + k % h
        e = (m & (h - 1)) << (s if dif else 3 - s)
        if e:
            out.append((m + h, 12 * e))
    return out


def addsub(x, h):
    for m in range(16):
        if not m & h:
            x[m], x[m + h] = (x[m] + x[m + h]) % P, (x[m] - x[m + h]) % P


def layer(x, w_s, j):
    return [x[m] * pow(w_s, j * brev4(m), P) % P for m in range(16)]


def dit16(x, w_s, j):
    x = layer(x, w_s, j)
    addsub(x, 1)
    for s in (1, 2, 3):
        for m, S in pow2_targets(s, False):
            x[m] = mul_pow2(x[m], S) % P
        addsub(x, 1 << s)
    return [x[13 * q & 15] for q in range(16)]     # DFT under g^13: output q is output 13 q of the DFT under g


def dif16(x, w_s_inv, j):
    x = list(x)
    for s in (0, 1, 2):
        addsub(x, 8 >> s)
        for m, S in pow2_targets(s, True):
            x[m] = mul_pow2(x[m], S) % P
    addsub(x, 1)
    x = [x[brev4(3 * brev4(m) & 15)] for m in range(16)]   # DFT under g^3; register m holds frequency brev4(m)
    return layer(x, w_s_inv, j)


def test_the_dft_twiddle_counts_are_those_the_kernel_groups():
    for dif in (False, True):
        ks = sorted(S // 12 for s in range(4) for _, S in pow2_targets(s, dif))
        assert ks == [1, 2, 2, 2, 3, 4, 4, 4, 4, 4, 4, 4, 5, 6, 6, 6, 7]


@pytest.mark.parametrize("L", [12, 13, 14])
@pytest.mark.parametrize("direction", ["dit", "dif"])
def test_layer_plus_shift_dft_equals_the_four_table_twiddle_stages(L, direction):
    rng = random.Random(100 * L + (direction == "dif"))
    rt = 4 if L % 4 == 0 else L % 4
    if direction == "dit":   # forward root; passes b = 0 (innermost), 4, 8 (the outermost one only when rt == 4)
        bs = [b for b in (0, 4, 8) if b + 4 <= L - rt] + ([L - 4] if rt == 4 else [])
        w_blk = root(L)
    else:                    # inverse root; passes b = L - 4, L - 8, ... > 0, and b = 0 when rt == 4
        bs = list(range(L - 4, 0, -4)) + ([0] if rt == 4 else [])
        w_blk = pow(root(L), P - 2, P)
    for b in sorted(set(bs)):
        sub = 1 << b
        w_s = pow(w_blk, 1 << (L - b - 4), P)      # the root of order S = 16 sub the block's table supplies
        lanes = {0, sub - 1, sub // 2} | {rng.randrange(sub) for _ in range(24)}
        for j in sorted(lanes):
            x = [rng.getrandbits(64) % P for _ in range(16)]
            if direction == "dit":
                assert dit16(x, w_s, j) == radix2_stages_dit(x, w_s, j, sub), (L, b, j)
            else:
                assert dif16(x, w_s, j) == radix2_stages_dif(x, w_s, j, sub), (L, b, j)


def test_layer_table_index_is_a_bijection_onto_its_rows():
    """lay[((16 + r) << b) + j]: the rows of all sub-block sizes 2^b, b <= L - 4, tile [16, 2^(L+1)) without overlap"""
    L = 12
    seen = set()
    for b in range(L - 3):
        for r in range(16):
            lo = (16 + r) << b
            cells = range(lo, lo + (1 << b))
            assert not seen.intersection((cells[0], cells[-1]))
            seen.update(cells)
    assert seen == set(range(16, 2 << L))
