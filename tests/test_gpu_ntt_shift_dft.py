"""GPU: the multiplications by 2^(12k) (gl::mul_pow2_n), the VALU NTT block kernels whose radix-16 passes are a twiddle
layer plus a shift-only 16-point DFT (csrc/ntt.hip, dit16 / dif16), and the proof-of-work search that stops at the
winner -- all exact, against Python integers and the CPU oracle."""
import numpy as np
import pytest

from util import (P, bitrev_perm, coset_major_to_natural, rand_field, to_dev, to_host)

pytestmark = pytest.mark.gpu


def test_mul_pow2_against_big_integers(bpg):
    """every k = 1..7, groups of four, groups of three and the one-element form; any u64 in (words >= p included)"""
    rng = np.random.default_rng(12)
    edge = [0, 1, 2, 7, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, P - 1, P, P + 1, (1 << 63), (1 << 64) - 1,
            (1 << 64) - (1 << 32), (1 << 64) - (1 << 32) - 1, 0xFFFFFFFF00000000, 0x00000000FFFFFFFF,
            0xFFFFFFFEFFFFFFFF, 0x8000000080000000, P - (1 << 32), (1 << 48) + 12345]
    a = list(edge)
    for k in range(1, 8):   # shifted limbs all ones / all zeros: the carry and borrow edges of every shift
        s = 12 * k % 32
        a += [((1 << 64) - 1) >> s, (((1 << 64) - 1) >> s) + 1, ((1 << (32 - s)) - 1) << 32, (1 << (64 - s)) - 1]
    a += [int(v) for v in rng.integers(0, 1 << 64, 4096, dtype=np.uint64)]
    a += [P + int(v) for v in rng.integers(0, (1 << 32) - 1, 64, dtype=np.uint64)]   # non-canonical words
    a += [(1 << 64) - 1] * 5    # n no multiple of four: the last group is padded
    out = to_host(bpg.ops.mul_pow2(to_dev(np.array(a, dtype=np.uint64))))
    assert out.shape == (21, len(a))
    for k in range(1, 8):
        want = np.array([(x << (12 * k)) % P for x in a], dtype=np.uint64)
        for f, name in enumerate(("groups of four", "groups of three", "one element")):
            bad = np.nonzero(out[3 * (k - 1) + f] != want)[0]
            assert bad.size == 0, (k, name, hex(a[bad[0]]), hex(int(out[3 * (k - 1) + f][bad[0]])), hex(int(want[bad[0]])))


_REF = {}


def reference(oracle, log_n, n_cols, rates):
    """one oracle run per shape, shared by the split modes: inputs are ANY u64, the oracle gets them reduced"""
    key = (log_n, n_cols)
    if key not in _REF:
        rng = np.random.default_rng(4000 + log_n)
        n = 1 << log_n
        raw = rng.integers(0, 1 << 64, size=(n_cols, n), dtype=np.uint64)
        raw[:, ::3] = np.uint64(2**64 - 1)            # all-ones and other words >= p, in both halves of every block
        raw[:, 1::5] = np.uint64(P)
        raw[:, n // 2 + 1::7] = np.uint64(P + 12345)
        raw[:, 2::4096] = np.uint64(P + 1)            # (every 2^12-point block, both halves)
        raw[:, 2048 + 5::4096] = np.uint64(2**64 - 2**32)
        red = raw % np.uint64(P)
        br = bitrev_perm(log_n)
        ref = {"raw": raw, "br": br,
               "coeffs": oracle.ntt_batch(red, inverse=True),               # raw as values: natural-order coefficients
               "vals": oracle.ntt_batch(red[:, br], inverse=False)}         # raw as bit-reversed coefficients: values
        for r in rates:
            c, lde = oracle.lde_batch(red, r)
            assert (c == ref["coeffs"]).all()
            ref["lde", r] = lde
            ref["lde_from_coeffs", r] = oracle.lde_batch(ref["vals"], r)[1]
        for v in ref.values():
            v.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


@pytest.fixture
def valu_kernels(bpg):
    with bpg.ops.tuned(ntt_mx=0):
        yield


@pytest.mark.parametrize("split", [1, 2])   # never / two workgroups per block wherever possible
@pytest.mark.parametrize("log_n,n_cols", [(12, 3), (13, 3), (14, 2)])
def test_valu_block_kernels_match_the_oracle(bpg, oracle, log_n, n_cols, split):
    with bpg.ops.tuned(ntt_mx=0, ntt_split=split):
        rates = (1, 3)
        ref = reference(oracle, log_n, n_cols, rates)
        raw, br = ref["raw"], ref["br"]
        # inverse, out of place (split eligible) and in place
        d = to_dev(raw.copy())
        got = to_host(bpg.ops.intt_batch(d))
        assert (to_host(d) == raw).all()
        assert (got[:, br] == ref["coeffs"]).all(), "inverse, out of place"
        got = to_host(bpg.ops.ntt_batch_(to_dev(raw.copy()), bpg.ops.NTT_INV_NAT2BR))
        assert (got[:, br] == ref["coeffs"]).all(), "inverse, in place"
        # forward
        got = to_host(bpg.ops.ntt_batch_(to_dev(raw.copy()), bpg.ops.NTT_FWD_BR2NAT))
        assert (got == ref["vals"]).all(), "forward"
        for r in rates:
            idx = coset_major_to_natural(log_n, r)
            coeffs, lde = bpg.ops.lde_batch(to_dev(raw.copy()), r)
            assert (to_host(coeffs)[:, br] == ref["coeffs"]).all(), ("lde: coefficients", r)
            assert (to_host(lde)[:, idx] == ref["lde", r]).all(), ("lde from values", r)
            _, lde = bpg.ops.lde_batch(to_dev(raw.copy()), r, from_coeffs=True)
            assert (to_host(lde)[:, idx] == ref["lde_from_coeffs", r]).all(), ("lde from coefficients", r)


def test_valu_block_kernels_under_a_global_pass(bpg, oracle, valu_kernels):
    """2^17 points: 2^13-point blocks and one global radix-16 pass, which keeps the table-twiddle butterflies"""
    log_n = 17
    ref = reference(oracle, log_n, 1, (1,))
    raw, br = ref["raw"], ref["br"]
    got = to_host(bpg.ops.ntt_batch_(to_dev(raw.copy()), bpg.ops.NTT_INV_NAT2BR))
    assert (got[:, br] == ref["coeffs"]).all()
    got = to_host(bpg.ops.ntt_batch_(to_dev(raw.copy()), bpg.ops.NTT_FWD_BR2NAT))
    assert (got == ref["vals"]).all()
    coeffs, lde = bpg.ops.lde_batch(to_dev(raw.copy()), 1)
    assert (to_host(coeffs)[:, br] == ref["coeffs"]).all()
    assert (to_host(lde)[:, coset_major_to_natural(log_n, 1)] == ref["lde", 1]).all()


def test_pow_grind_finds_the_smallest_witness_of_a_host_scan(bpg, oracle):
    """10 bits: the winner sits about 2^10 candidates into a launch of many workgroups, which now leave once a smaller
    witness is known; the result must stay the minimum"""
    rng = np.random.default_rng(510)
    bits, scan = 10, 1 << 14
    for pos in (0, 3, 5, 7):
        state = rand_field(rng, (12,))
        tries = np.tile(state, (scan, 1))
        tries[:, pos] = np.arange(scan, dtype=np.uint64)
        ok = (oracle.poseidon(tries)[:, 7] >> np.uint64(64 - bits)) == 0
        assert ok.any(), "no witness among the first 2^14 candidates (probability e^-16)"
        assert bpg.ops.pow_grind(state, pos, bits) == int(np.argmax(ok)), pos
