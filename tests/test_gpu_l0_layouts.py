"""The L0 entry points at the buffer layouts include/bpg.h promises ("Buffers of the L0 entries"): column strides wider
than the column, in-place calls, exact-size outputs, refused arguments.  Every buffer lies between poisoned guards
(tests/layout_harness.py); after each call the whole allocation is compared bit for bit: the oracle's (or Python
integers') words in the column bodies, every other word as it was.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from layout_harness import POISON_IN, POISON_OUT, UNWRITTEN, Guarded, Layout
from util import P, bitrev_perm, coset_major_to_natural, rand_field

pytestmark = pytest.mark.gpu

INVALID = -2   # BP_ERR_INVALID_INPUT
MAX_COLS = 65535   # BP_NTT_MAX_COLS
U64 = np.uint64


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def raw_words(rng, shape):
    """any u64 (bpg.h: reduced mod p on the way in), with words >= p all along every column"""
    raw = rng.integers(0, 1 << 64, size=shape, dtype=U64)
    raw[..., ::3] = U64(2**64 - 1)
    raw[..., 1::5] = U64(P)
    raw[..., 2::7] = U64(P + 12345)
    return raw


def ext_pair(v):
    return (C.c_uint64 * 2)(int(v[0]), int(v[1]))


# ------------------------------------------------------------------------------------------------ K2 under strides

# the smallest shapes that reach each path of plan_ntt (csrc/ntt.hip): generic LDS kernel (short block, full block);
# 16-per-lane / matrix-core blocks of 2^12, 2^13, 2^14 (nine columns: a padded last group of eight on the XCD-aware
# grids); one register pass over 2^12- / 2^13-point blocks; the 6- and 8-stage tile passes; a register pass on top
K2_SHAPES = [(3, 5), (9, 7), (12, 3), (13, 3), (14, 9), (15, 2), (17, 2), (18, 2), (21, 1), (23, 1)]
NTT_FORMS = [(split, mx) for split in (1, 2, 0) for mx in (0, 3)]   # as test_ntt_takes_any_u64_in_every_kernel_form

_K2_REF = {}


def k2_ref(oracle, log_n, n_cols):
    """raw input, its residues, and the oracle's forward / inverse transforms of them (natural order); computed once per
    shape and shared (kept for the shapes more than one test uses)"""
    key = (log_n, n_cols)
    if key in _K2_REF:
        return _K2_REF[key]
    rng = np.random.default_rng(1000 + log_n)
    raw = raw_words(rng, (n_cols, 1 << log_n))
    red = raw % U64(P)
    ref = {"raw": raw, "red": red, "br": bitrev_perm(log_n), "fwd": oracle.ntt_batch(red, inverse=False),
           "inv": oracle.ntt_batch(red, inverse=True)}
    for v in ref.values():
        v.setflags(write=False)
    if log_n <= 21:
        _K2_REF[key] = ref
    return ref


def strides_of(n):
    return (n + 1, n + 8, 2 * n)    # columns only 8-byte aligned / a few words apart / a column apart


@pytest.mark.parametrize("log_n,n_cols", K2_SHAPES)
def test_ntt_batch_under_strides(bpg, oracle, log_n, n_cols):
    """bp_ntt_batch, all four directions, in place at three strides, in every kernel form; half the calls on raw u64
    words.  Column bodies = the oracle's transform of the residues, pads and guards untouched."""
    ref = k2_ref(oracle, log_n, n_cols)
    n, br, L = 1 << log_n, ref["br"], bpg.lib()
    want_live = {0: ref["fwd"], 1: ref["inv"][:, br], 2: ref["fwd"], 3: ref["inv"]}
    made = None
    for si, stride in enumerate(strides_of(n)):
        if made is None or n_cols > 1:    # one column: the image does not depend on the stride
            lay = Layout(n_cols, n, stride)
            bufs = {(order, k): Guarded("d_cols", lay, x[:, br] if order == "br" else x, POISON_IN)
                    for order in ("nat", "br") for k, x in enumerate((ref["red"], ref["raw"]))}
            made = bufs, {d: bufs["nat", 0].expect(w) for d, w in want_live.items()}
        bufs, want = made
        for fi, (split, mx) in enumerate(NTT_FORMS):
            with bpg.ops.tuned(ntt_split=split, ntt_mx=mx):
                for d in range(4):
                    k = (fi + d + si) & 1
                    g = bufs["br" if d == 0 else "nat", k]
                    bpg._lib.check(L.bp_ntt_batch(g.fresh(), log_n, n_cols, stride, d, _stream()))
                    g.check(want[d], "dir %d, stride %d, ntt_split=%d, ntt_mx=%d, %s words" % (d, stride, split, mx, ("canonical", "raw")[k]))


@pytest.mark.parametrize("log_n,n_cols", K2_SHAPES[:-1])
def test_intt_batch_under_strides(bpg, oracle, log_n, n_cols):
    """bp_intt_batch out of place with unequal strides (input untouched, pads of both untouched) and in place."""
    ref = k2_ref(oracle, log_n, n_cols)
    n, br, L = 1 << log_n, ref["br"], bpg.lib()
    coeffs = ref["inv"][:, br]
    for si, (s_in, s_out) in enumerate(((n + 1, 2 * n), (2 * n, n + 8), (n + 8, n + 1))):
        ins = [Guarded("d_values", Layout(n_cols, n, s_in), x, POISON_IN) for x in (ref["red"], ref["raw"])]
        out = Guarded("d_coeffs_out", Layout(n_cols, n, s_out), UNWRITTEN, POISON_OUT)
        want_out, want_in_place = out.expect(coeffs), ins[0].expect(coeffs)
        for fi, (split, mx) in enumerate(NTT_FORMS):
            with bpg.ops.tuned(ntt_split=split, ntt_mx=mx):
                k = (fi + si) & 1
                what = "strides %d -> %d, ntt_split=%d, ntt_mx=%d, %s words" % (s_in, s_out, split, mx, ("canonical", "raw")[k])
                bpg._lib.check(L.bp_intt_batch(ins[k].fresh(), s_in, out.fresh(), s_out, log_n, n_cols, _stream()))
                out.check(want_out, what)
                ins[k].check(None, what)
                p = ins[1 - k].fresh()
                bpg._lib.check(L.bp_intt_batch(p, s_in, p, s_in, log_n, n_cols, _stream()))
                ins[1 - k].check(want_in_place, "in place, " + what)


LDE_MODES = ("values, separate coefficients", "values, in place", "coefficients, no copy", "coefficients, copied")


@pytest.mark.parametrize("rate_bits", [1, 3])
@pytest.mark.parametrize("log_n,n_cols", [s for s in K2_SHAPES if s[0] <= 18])
def test_lde_batch_under_strides(bpg, oracle, log_n, n_cols, rate_bits):
    """bp_lde_batch from values (separate coefficient buffer / in place) and from coefficients (null coefficient
    buffer / a separate one: the copy), each with three different strides, in every kernel form."""
    ref = k2_ref(oracle, log_n, n_cols)
    n, br, L = 1 << log_n, ref["br"], bpg.lib()
    m = n << rate_bits
    idx = coset_major_to_natural(log_n, rate_bits)

    def coset_major(nat):
        cm = np.empty_like(nat)
        cm[:, idx] = nat
        return cm
    c_nat, lde_nat = oracle.lde_batch(ref["red"], rate_bits)
    assert (c_nat == ref["inv"]).all()
    lde_a, coeffs_a = coset_major(lde_nat), c_nat[:, br]
    c_raw = raw_words(np.random.default_rng(2000 + log_n), (n_cols, n))    # as stored: bit-reversed
    c_red = c_raw % U64(P)
    lde_b = coset_major(oracle.lde_batch(c_red[:, br], rate_bits, from_coeffs=True)[1])
    for si, (s_in, s_c, s_l) in enumerate(((n + 1, n + 8, m + 1), (n + 8, 2 * n, 2 * m), (2 * n, n + 1, m + 8))):
        in_a = [Guarded("d_in", Layout(n_cols, n, s_in), x, POISON_IN) for x in (ref["red"], ref["raw"])]
        in_b = [Guarded("d_in", Layout(n_cols, n, s_in), x, POISON_IN) for x in (c_red, c_raw)]
        co = Guarded("d_coeffs_out", Layout(n_cols, n, s_c), UNWRITTEN, POISON_OUT)
        lde = Guarded("d_lde_out", Layout(n_cols, m, s_l), UNWRITTEN, POISON_OUT)
        want_co_a, want_co_b, want_in_place = co.expect(coeffs_a), co.expect(c_red), in_a[0].expect(coeffs_a)
        want_lde = lde.expect(lde_a), lde.expect(lde_b)
        for fi, (split, mx) in enumerate(NTT_FORMS):
            with bpg.ops.tuned(ntt_split=split, ntt_mx=mx):
                for mode, name in enumerate(LDE_MODES):
                    k = (fi + si + mode) & 1
                    what = "%s; strides %d, %d, %d; ntt_split=%d, ntt_mx=%d, %s words" % (name, s_in, s_c, s_l, split, mx, ("canonical", "raw")[k])
                    src = (in_b if mode >= 2 else in_a)[k]
                    p_in, p_lde = src.fresh(), lde.fresh()
                    if mode == 1:
                        rc = L.bp_lde_batch(p_in, s_in, p_in, s_in, p_lde, s_l, log_n, rate_bits, n_cols, 0, _stream())
                    elif mode == 2:
                        rc = L.bp_lde_batch(p_in, s_in, None, 0, p_lde, s_l, log_n, rate_bits, n_cols, 1, _stream())
                    else:
                        rc = L.bp_lde_batch(p_in, s_in, co.fresh(), s_c, p_lde, s_l, log_n, rate_bits, n_cols, int(mode == 3), _stream())
                    bpg._lib.check(rc)
                    lde.check(want_lde[mode >= 2], what)
                    src.check(want_in_place if mode == 1 else None, what)
                    if mode in (0, 3):
                        co.check(want_co_b if mode == 3 else want_co_a, what)


# ------------------------------------------------------------------------------------------------ the contract holes

class Arena:
    """one guarded allocation a refused call's pointers all lie in: it must come back as it was"""

    def __init__(self, words, seed):
        self.g = Guarded("arena", Layout(1, words), rand_field(np.random.default_rng(seed), (1, words)), POISON_IN)
        self.base = self.g.fresh()

    def at(self, word):
        return self.base + 8 * word


def refused(bpg, entry, rc, *arenas):
    import torch
    assert rc == INVALID, "%s returned %d (%s)" % (entry, rc, bpg._lib.STATUS_NAMES.get(rc))
    assert entry.encode() in bpg.lib().bp_last_error(), bpg.lib().bp_last_error()
    torch.cuda.synchronize()
    for a in arenas:
        a.g.check(None, "after %s refused the call" % entry)


def test_the_same_pointer_with_two_strides_is_refused(bpg, oracle):
    """d_values == d_coeffs_out with in_stride = n, out_stride = 2n used to pass the overlap test (equal pointers are in
    place) and return BP_OK with column 1's coefficients written over column 2's values before they were read.  Refused
    now, by bp_intt_batch and by bp_lde_batch for d_coeffs_out == d_in; in place with EQUAL strides > n stays legal."""
    log_n, n_cols, L = 4, 3, bpg.lib()
    n = 1 << log_n
    a, b = Arena(8 * n, 31), Arena(32 * n, 32)
    for s_in, s_out in ((n, 2 * n), (2 * n, n), (n + 1, n)):
        refused(bpg, "bp_intt_batch", L.bp_intt_batch(a.base, s_in, a.base, s_out, log_n, n_cols, _stream()), a)
        for from_coeffs in (0, 1):
            refused(bpg, "bp_lde_batch", L.bp_lde_batch(a.base, s_in, a.base, s_out, b.base, 2 * n, log_n, 1, n_cols,
                                                        from_coeffs, _stream()), a, b)
    vals = rand_field(np.random.default_rng(33), (n_cols, n))
    br = bitrev_perm(log_n)
    c_nat, lde_nat = oracle.lde_batch(vals, 1)
    g = Guarded("d_values", Layout(n_cols, n, 2 * n), vals, POISON_IN)
    p = g.fresh()
    bpg._lib.check(L.bp_intt_batch(p, 2 * n, p, 2 * n, log_n, n_cols, _stream()))
    g.check(g.expect(c_nat[:, br]), "in place, stride 2n")
    lde = Guarded("d_lde_out", Layout(n_cols, 2 * n, 2 * n + 3), UNWRITTEN, POISON_OUT)
    p = g.fresh()
    bpg._lib.check(L.bp_lde_batch(p, 2 * n, p, 2 * n, lde.fresh(), 2 * n + 3, log_n, 1, n_cols, 0, _stream()))
    g.check(g.expect(c_nat[:, br]), "LDE in place, stride 2n")
    cm = np.empty_like(lde_nat)
    cm[:, coset_major_to_natural(log_n, 1)] = lde_nat
    lde.check(lde.expect(cm), "LDE in place, stride 2n")


def test_overlapping_buffers_are_refused(bpg, oracle):
    """input and output partially overlapping, in both orders (bp_intt_batch; bp_lde_batch's input and coefficients);
    an LDE output over the coefficients it is computed from; touching buffers are not overlapping."""
    log_n, n_cols, L = 5, 3, bpg.lib()
    n = 1 << log_n
    span = 2 * (n + 2) + n                                  # three columns at stride n + 2
    a, b = Arena(16 * n, 41), Arena(16 * n, 42)
    for lo, hi in ((0, n // 2), (0, span - 1), (0, n + 1), (5, 4)):   # second buffer `hi` words into the arena, first at `lo`
        for x, y in ((lo, hi), (hi, lo)):
            refused(bpg, "bp_intt_batch", L.bp_intt_batch(a.at(x), n + 2, a.at(y), n + 2, log_n, n_cols, _stream()), a)
            refused(bpg, "bp_lde_batch", L.bp_lde_batch(a.at(x), n + 2, a.at(y), n + 2, b.base, 2 * n, log_n, 1, n_cols, 0, _stream()), a, b)
            refused(bpg, "bp_lde_batch", L.bp_lde_batch(a.at(x), n + 2, a.at(y), n + 2, b.base, 2 * n, log_n, 1, n_cols, 1, _stream()), a, b)
    # the LDE output on the coefficients the forward transform reads: the input (from_coeffs) or the coefficient buffer
    # (the LDE's three columns at stride 2n span 6n words)
    for off in (0, n // 2, span - 1):
        refused(bpg, "bp_lde_batch", L.bp_lde_batch(a.base, n + 2, None, 0, a.at(off), 2 * n, log_n, 1, n_cols, 1, _stream()), a)
        refused(bpg, "bp_lde_batch", L.bp_lde_batch(b.base, n + 2, a.base, n + 2, a.at(off), 2 * n, log_n, 1, n_cols, 0, _stream()), a, b)
    for back in (6 * n - 1, 3 * n, 1):   # the LDE output starts before them and reaches in
        refused(bpg, "bp_lde_batch", L.bp_lde_batch(a.at(8 * n), n + 2, None, 0, a.at(8 * n - back), 2 * n, log_n, 1, n_cols, 1, _stream()), a)
        refused(bpg, "bp_lde_batch", L.bp_lde_batch(b.base, n + 2, a.at(8 * n), n + 2, a.at(8 * n - back), 2 * n, log_n, 1, n_cols, 0, _stream()), a, b)
    # touching is not overlapping: the output starts on the word after the input's last
    vals = rand_field(np.random.default_rng(43), (n_cols, n))
    want = oracle.ntt_batch(vals, inverse=True)[:, bitrev_perm(log_n)]
    lay = Layout(1, 2 * span)
    img = np.full((1, 2 * span), POISON_IN, dtype=U64)
    after = img.copy()
    for c in range(n_cols):
        img[0, c * (n + 2):c * (n + 2) + n] = vals[c]
        after[0, c * (n + 2):c * (n + 2) + n] = vals[c]
        after[0, span + c * (n + 2):span + c * (n + 2) + n] = want[c]
    g = Guarded("input then output", lay, img, POISON_IN)
    p = g.fresh()
    bpg._lib.check(L.bp_intt_batch(p, n + 2, p + 8 * span, n + 2, log_n, n_cols, _stream()))
    g.check(g.expect(after), "output right behind the input")


def test_short_strides_and_null_pointers_are_refused(bpg):
    """a stride shorter than the column, in every entry that takes one; a null pointer in every pointer argument.
    BP_ERR_INVALID_INPUT, bp_last_error() names the entry, nothing is written."""
    log_n, n_cols, L, st = 4, 3, bpg.lib(), _stream()
    n = 1 << log_n
    a, b, c = Arena(16 * n, 51), Arena(16 * n, 52), Arena(16 * n, 53)
    z = ext_pair((3, 5))
    for d in range(4):
        refused(bpg, "bp_ntt_batch", L.bp_ntt_batch(a.base, log_n, n_cols, n - 1, d, st), a)
        refused(bpg, "bp_ntt_batch", L.bp_ntt_batch(None, log_n, n_cols, n, d, st))
    refused(bpg, "bp_ntt_batch", L.bp_ntt_batch(a.base, log_n, n_cols, 0, 1, st), a)
    refused(bpg, "bp_intt_batch", L.bp_intt_batch(a.base, n - 1, b.base, n, log_n, n_cols, st), a, b)
    refused(bpg, "bp_intt_batch", L.bp_intt_batch(a.base, n, b.base, n - 1, log_n, n_cols, st), a, b)
    refused(bpg, "bp_intt_batch", L.bp_intt_batch(None, n, b.base, n, log_n, n_cols, st), b)
    refused(bpg, "bp_intt_batch", L.bp_intt_batch(a.base, n, None, n, log_n, n_cols, st), a)
    for fc in (0, 1):
        refused(bpg, "bp_lde_batch", L.bp_lde_batch(a.base, n - 1, b.base, n, c.base, 2 * n, log_n, 1, n_cols, fc, st), a, b, c)
        refused(bpg, "bp_lde_batch", L.bp_lde_batch(a.base, n, b.base, n - 1, c.base, 2 * n, log_n, 1, n_cols, fc, st), a, b, c)
        refused(bpg, "bp_lde_batch", L.bp_lde_batch(a.base, n, b.base, n, c.base, 2 * n - 1, log_n, 1, n_cols, fc, st), a, b, c)
        refused(bpg, "bp_lde_batch", L.bp_lde_batch(None, n, b.base, n, c.base, 2 * n, log_n, 1, n_cols, fc, st), b, c)
        refused(bpg, "bp_lde_batch", L.bp_lde_batch(a.base, n, b.base, n, None, 2 * n, log_n, 1, n_cols, fc, st), a, b)
    refused(bpg, "bp_lde_batch", L.bp_lde_batch(a.base, n, None, n, c.base, 2 * n, log_n, 1, n_cols, 0, st), a, c)
    refused(bpg, "bp_poseidon_perm_batch", L.bp_poseidon_perm_batch(None, 4, st))
    # bp_merkle_commit: 2n rows
    refused(bpg, "bp_merkle_commit", L.bp_merkle_commit(a.base, 2 * n - 1, n_cols, log_n, 1, 2, b.base, st), a, b)
    refused(bpg, "bp_merkle_commit", L.bp_merkle_commit(None, 2 * n, n_cols, log_n, 1, 2, b.base, st), b)
    refused(bpg, "bp_merkle_commit", L.bp_merkle_commit(a.base, 2 * n, n_cols, log_n, 1, 2, None, st), a)
    refused(bpg, "bp_openings", L.bp_openings(a.base, n - 1, log_n, n_cols, z, z, b.base, c.base, st), a, b, c)
    refused(bpg, "bp_openings", L.bp_openings(None, n, log_n, n_cols, z, z, b.base, c.base, st), b, c)
    refused(bpg, "bp_openings", L.bp_openings(a.base, n, log_n, n_cols, None, z, b.base, c.base, st), a, b, c)
    refused(bpg, "bp_openings", L.bp_openings(a.base, n, log_n, n_cols, z, z, None, c.base, st), a, c)
    refused(bpg, "bp_openings", L.bp_openings(a.base, n, log_n, n_cols, z, z, b.base, None, st), a, b)
    refused(bpg, "bp_fri_fold", L.bp_fri_fold(None, log_n, 1, 4, 7, z, b.base, st), b)
    refused(bpg, "bp_fri_fold", L.bp_fri_fold(a.base, log_n, 1, 4, 7, None, b.base, st), a, b)
    refused(bpg, "bp_fri_fold", L.bp_fri_fold(a.base, log_n, 1, 4, 7, z, None, st), a)
    state, nonce = (C.c_uint64 * 12)(*range(12)), C.c_uint64(0x1234)
    refused(bpg, "bp_pow_grind", L.bp_pow_grind(None, 0, 8, C.byref(nonce), st))
    refused(bpg, "bp_pow_grind", L.bp_pow_grind(state, 0, 8, None, st))
    assert nonce.value == 0x1234


def test_column_limit(bpg, oracle):
    """The K2 kernels index columns by grid.y: BP_NTT_MAX_COLS = 65535 columns per call work (oracle's values), one
    more -- here 65536 + 3 -- is refused before anything is launched, never handed to the runtime."""
    log_n, L, st = 2, bpg.lib(), _stream()
    n = 1 << log_n
    over = 65536 + 3
    a, b, c = Arena(over * n, 61), Arena(over * n, 62), Arena(over * 2 * n, 63)
    for d in range(4):
        refused(bpg, "bp_ntt_batch", L.bp_ntt_batch(a.base, log_n, over, n, d, st), a)
    refused(bpg, "bp_intt_batch", L.bp_intt_batch(a.base, n, b.base, n, log_n, over, st), a, b)
    refused(bpg, "bp_intt_batch", L.bp_intt_batch(a.base, n, a.base, n, log_n, over, st), a)
    for fc in (0, 1):
        refused(bpg, "bp_lde_batch", L.bp_lde_batch(a.base, n, b.base, n, c.base, 2 * n, log_n, 1, over, fc, st), a, b, c)
    assert b"65535" in L.bp_last_error()
    refused(bpg, "bp_ntt_batch", L.bp_ntt_batch(a.base, log_n, MAX_COLS + 1, n, 0, st), a)
    # the limit itself
    raw = raw_words(np.random.default_rng(64), (MAX_COLS, n))
    red, br = raw % U64(P), bitrev_perm(log_n)
    fwd, inv = oracle.ntt_batch(red, inverse=False), oracle.ntt_batch(red, inverse=True)
    s = n + 1
    g = Guarded("d_cols", Layout(MAX_COLS, n, s), raw, POISON_IN)
    g_br = Guarded("d_cols", Layout(MAX_COLS, n, s), raw[:, br], POISON_IN)
    for d, w in enumerate((fwd, inv[:, br], fwd, inv)):
        src = g_br if d == 0 else g
        bpg._lib.check(L.bp_ntt_batch(src.fresh(), log_n, MAX_COLS, s, d, st))
        src.check(g.expect(w), "dir %d, 65535 columns" % d)
    out = Guarded("d_coeffs_out", Layout(MAX_COLS, n, n), UNWRITTEN, POISON_OUT)
    bpg._lib.check(L.bp_intt_batch(g.fresh(), s, out.fresh(), n, log_n, MAX_COLS, st))
    out.check(out.expect(inv[:, br]), "65535 columns")
    g.check(None, "65535 columns")
    lde = Guarded("d_lde_out", Layout(MAX_COLS, 2 * n, 2 * n + 1), UNWRITTEN, POISON_OUT)
    cm = np.empty((MAX_COLS, 2 * n), dtype=U64)
    cm[:, coset_major_to_natural(log_n, 1)] = oracle.lde_batch(red, 1)[1]
    bpg._lib.check(L.bp_lde_batch(g.fresh(), s, out.fresh(), n, lde.fresh(), 2 * n + 1, log_n, 1, MAX_COLS, 0, st))
    lde.check(lde.expect(cm), "65535 columns")
    out.check(out.expect(inv[:, br]), "LDE of 65535 columns")
    g.check(None, "LDE of 65535 columns")


# ------------------------------------------------------------------------------------------------ K4, K3, K6, K8

MERKLE_SHAPES = [(3, 1, 3, 4), (4, 0, 9, 2), (7, 3, 19, 4), (10, 1, 135, 0), (12, 1, 33, 2)]
_MERKLE_REF = {}


def merkle_ref(oracle, shape):
    if shape not in _MERKLE_REF:
        log_n, rate_bits, n_cols, cap_h = shape
        lde_cm = rand_field(np.random.default_rng(3000 + log_n), (n_cols, 1 << (log_n + rate_bits)))
        nat = np.ascontiguousarray(lde_cm[:, coset_major_to_natural(log_n, rate_bits)])
        _MERKLE_REF[shape] = lde_cm, oracle.merkle_commit(nat, cap_h, bitrev_rows=True)[0].reshape(1, -1).copy()
    return _MERKLE_REF[shape]


@pytest.mark.parametrize("form", ["quad", "lane", "mx4", "mx2", "mx1", "mx", "mx+fused", "mx+fused+wide", "quad+fused",
                                  "mx4-ungrouped"])
def test_merkle_commit_under_strides(bpg, oracle, form):
    """bp_merkle_commit reading columns lde_stride apart, into a digest buffer of exactly bp_merkle_digest_words words,
    in the forms of test_merkle_commit_matches_oracle."""
    L = bpg.lib()
    for shape in MERKLE_SHAPES:
        log_n, rate_bits, n_cols, cap_h = shape
        knobs = {"quad_threshold": (1 << 40) if form.startswith("quad") else 1,
                 "poseidon_mx": 1 if form.startswith("mx") else 0,
                 "merkle_fused": 1 if "+fused" in form else 0}
        if form[:3] in ("mx4", "mx2", "mx1"):
            knobs["poseidon_mx_sets"] = int(form[2:3])
        if form.endswith("+wide"):
            knobs["merkle_wide"] = 14
        if form.endswith("-ungrouped"):
            knobs["poseidon_grouped"] = 0
        if form in ("mx", "mx+fused", "mx+fused+wide"):
            knobs["quad_threshold"] = 1 << (log_n + rate_bits)
        lde_cm, want_dig = merkle_ref(oracle, shape)
        rows = 1 << (log_n + rate_bits)
        words = int(L.bp_merkle_digest_words(log_n + rate_bits, cap_h))
        assert words == want_dig.size
        dig = Guarded("d_digests", Layout(1, words), UNWRITTEN, POISON_OUT)
        want = dig.expect(want_dig)
        for stride in (rows + 1, 2 * rows):
            lde = Guarded("d_lde", Layout(n_cols, rows, stride), lde_cm, POISON_IN)
            with bpg.ops.tuned(**knobs):
                bpg._lib.check(L.bp_merkle_commit(lde.fresh(), stride, n_cols, log_n, rate_bits, cap_h, dig.fresh(), _stream()))
            what = "%s, shape %s, lde_stride %d" % (form, shape, stride)
            dig.check(want, what)
            lde.check(None, what)


@pytest.mark.parametrize("form", ["mx4", "mx4-ungrouped", "mx2", "mx1", "lane"])
def test_poseidon_perm_batch_between_guards(bpg, oracle, form):
    """bp_poseidon_perm_batch on n states with poison right before the first and right after the last: the clamped tail of
    the matrix-core forms (16 states per set) and of the lane form (256 per workgroup) stays inside."""
    knobs = {"poseidon_mx": 0} if form == "lane" else {"poseidon_mx_sets": int(form[2:3])}
    if form.endswith("-ungrouped"):
        knobs["poseidon_grouped"] = 0
    rng = np.random.default_rng(70)
    for n in (1, 15, 17, 63, 65, 257):
        s = rand_field(rng, (n, 12))
        s[n // 2, ::2] = U64(2**64 - 1)       # inputs in [p, 2^64) behave as their residues
        g = Guarded("d_states", Layout(1, 12 * n), s.reshape(1, -1), POISON_IN)
        with bpg.ops.tuned(**knobs):
            bpg._lib.check(bpg.lib().bp_poseidon_perm_batch(g.fresh(), n, _stream()))
        g.check(g.expect(oracle.poseidon(s % U64(P)).reshape(1, -1)), "%s, %d states" % (form, n))


@pytest.mark.parametrize("log_nl,rate_bits", [(4, 1), (5, 3), (9, 3)])
def test_fri_fold_between_guards(bpg, oracle, log_nl, rate_bits):
    """bp_fri_fold: layer and next layer of exactly their sizes between guards, at three domain shifts; the input stays."""
    rng = np.random.default_rng(4000 + log_nl)
    log_m = log_nl + rate_bits
    m = 1 << log_m
    vals = rand_field(rng, (m, 2))                         # natural order: index i <-> shift * w_m^i
    beta = rand_field(rng, (2,))
    cm = np.empty_like(vals)
    cm[coset_major_to_natural(log_nl, rate_bits)] = vals
    src = Guarded("d_values", Layout(1, 2 * m), cm.reshape(1, -1), POISON_IN)
    out = Guarded("d_out", Layout(1, 2 * (m >> 4)), UNWRITTEN, POISON_OUT)
    for shift in (7, pow(7, 16, P), pow(7, 256, P)):
        want_br = oracle.fri_fold(vals[bitrev_perm(log_m)], 4, shift, beta)     # [m / 16, 2], bit-reversed order
        want = np.empty_like(want_br)
        want[coset_major_to_natural(log_nl - 4, rate_bits)] = want_br[bitrev_perm(log_m - 4)]
        bpg._lib.check(bpg.lib().bp_fri_fold(src.fresh(), log_nl, rate_bits, 4, shift, ext_pair(beta), out.fresh(), _stream()))
        out.check(out.expect(want.reshape(1, -1)), "shift %d" % shift)
        src.check(None, "shift %d" % shift)


def horner(c, z):
    """the polynomial with coefficients c (natural order) at z in F_p[X] / (X^2 - 7), on Python integers"""
    a0 = a1 = 0
    z0, z1 = int(z[0]), int(z[1])
    for v in reversed([int(x) for x in c]):
        a0, a1 = (a0 * z0 + 7 * a1 * z1 + v) % P, (a0 * z1 + a1 * z0) % P
    return a0, a1


def openings_case(bpg, log_n, coeffs, z0, z1, what):
    """coeffs: [n_cols, n] natural order.  Strides n + 1 and 2n, the power-vector scratch exactly 4 << log_n words, the
    result exactly 4 * n_cols words, all between guards; against Horner's rule."""
    n_cols, n = coeffs.shape
    stored = np.ascontiguousarray(coeffs[:, bitrev_perm(log_n)])
    want = np.array([horner(c, z0) + (horner(c, z1) if z1 is not None else (0, 0)) for c in coeffs], dtype=U64)
    pw = Guarded("d_pw_scratch", Layout(1, 4 << log_n), UNWRITTEN, POISON_OUT)
    out = Guarded("d_out", Layout(1, 4 * n_cols), UNWRITTEN, POISON_OUT)
    for stride in (n + 1, 2 * n):
        src = Guarded("d_coeffs", Layout(n_cols, n, stride), stored, POISON_IN)
        bpg._lib.check(bpg.lib().bp_openings(src.fresh(), stride, log_n, n_cols, ext_pair(z0), ext_pair(z1) if z1 is not None else None,
                                             pw.fresh(), out.fresh(), _stream()))
        out.check(out.expect(want.reshape(1, -1)), "%s, stride %d" % (what, stride))
        pw.check(None, "%s, stride %d" % (what, stride), scratch=True)
        src.check(None, "%s, stride %d" % (what, stride))


@pytest.mark.parametrize("log_n", [0, 8, 14])
def test_openings_under_strides(bpg, log_n):
    """bp_openings on random columns at two random points, and at one point (the second pair is written as zero)."""
    rng = np.random.default_rng(6000 + log_n)
    coeffs = rand_field(rng, (3, 1 << log_n))
    z0, z1 = rand_field(rng, (2,)), rand_field(rng, (2,))
    openings_case(bpg, log_n, coeffs, z0, z1, "two points")
    openings_case(bpg, log_n, coeffs, z0, None, "one point")


def test_openings_with_the_accumulator_at_its_fastest_wrap_rate(bpg):
    """2^14 coefficients per column = 64 terms per lane, every term as large as the field allows: columns of p - 1
    (which is 0xFFFFFFFF00000000: the all-ones high half), alone and alternating with the other extremes, at
    z0 = (p - 1, 0) and z1 = (p - 1, p - 1), whose powers keep both components at +-1-sized residues of p: gl::DotAcc's
    wrap counters advance on every product for the whole column."""
    log_n = 14
    n = 1 << log_n
    cols = np.empty((5, n), dtype=U64)
    cols[0] = P - 1
    cols[1] = 0xFFFFFFFF00000000
    cols[2, ::2], cols[2, 1::2] = P - 1, 0xFFFFFFFF00000000
    cols[3, ::2], cols[3, 1::2] = P - 1, 0xFFFFFFFF
    cols[4, ::2], cols[4, 1::2] = 0, P - 1
    openings_case(bpg, log_n, cols, (P - 1, 0), (P - 1, P - 1), "extreme columns")


# ------------------------------------------------------------------------------------------------ K9

POW_FORMS = ({}, {"poseidon_grouped": 0}, {"poseidon_mx": 0})   # grouped matrix-core (default) / ungrouped / one lane per state


def smallest_nonce(oracle, state, pos, bits, limit):
    """exhaustive search with the oracle's permutation; None if there is none below `limit`"""
    for lo in range(0, limit, 4096):
        tries = np.tile(np.asarray(state, dtype=U64), (min(4096, limit - lo), 1))
        tries[:, pos] = np.arange(lo, lo + len(tries), dtype=U64)
        ok = (oracle.poseidon(tries)[:, 7] >> U64(64 - bits)) == 0
        if ok.any():
            return lo + int(np.flatnonzero(ok)[0])
    return None


def grind_in_every_form(bpg, state, pos, bits):
    got = []
    for knobs in POW_FORMS:
        with bpg.ops.tuned(**knobs):
            got.append(bpg.ops.pow_grind(state, pos, bits))
    return got


@pytest.mark.parametrize("bits", [6, 10])
def test_pow_grind_at_every_rate_word_in_every_form(bpg, oracle, bits):
    """the nonce goes into rate word pos = 0..7: the matrix-core kernels' lane-to-word mapping for each of them, the
    ungrouped form and the lane form stand-alone; all return the smallest witness."""
    rng = np.random.default_rng(8000 + bits)
    for pos in range(8):
        state = rand_field(rng, (12,))
        want = smallest_nonce(oracle, state, pos, bits, 64 << bits)
        assert want is not None
        assert grind_in_every_form(bpg, state, pos, bits) == [want] * len(POW_FORMS), (pos, bits)


@pytest.mark.parametrize("seed,first,end", [(7005, 8192, 24576), (7271, 24576, 57344)])
def test_pow_grind_winner_beyond_the_first_launch(bpg, oracle, seed, first, end):
    """bp_pow_grind at 12 bits searches [0, 8192), then [8192, 24576), then [24576, 57344) (a first launch of
    max(4096, 2 * 2^bits) candidates, doubling): states (found by exhaustive search, fixed by their rng seed) whose
    smallest witness lies in the second and in the third launch, so the carried base is exercised."""
    bits, pos = 12, seed % 8
    state = rand_field(np.random.default_rng(seed), (12,))
    want = smallest_nonce(oracle, state, pos, bits, end)
    assert want is not None and first <= want < end, "the state no longer has its winner in [%d, %d): %s" % (first, end, want)
    assert grind_in_every_form(bpg, state, pos, bits) == [want] * len(POW_FORMS)


def test_pow_grind_argument_checks(bpg):
    L = bpg.lib()
    state = (C.c_uint64 * 12)(*range(1, 13))
    for pos, bits in ((8, 8), (0, 0), (0, 41), (0xFFFFFFFF, 8)):
        nonce = C.c_uint64(0x5EED)
        refused(bpg, "bp_pow_grind", L.bp_pow_grind(state, pos, bits, C.byref(nonce), _stream()))
        assert nonce.value == 0x5EED
