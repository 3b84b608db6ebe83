"""tests/lazy_operands.py held to its own claims, on the host: the device-form models against Python integers, the
generators against the conditions the GPU tests rely on (how often they reach the upper representative, counted with
the models), the integer Poseidon against the oracle and against its own inverse.  The counts are conditions on the
INPUTS: a count that falls short means the inputs are wrong, not the bar."""
import numpy as np
import pytest

import lazy_operands as lo
from lazy_operands import P
from util import rand_field

LOG_N = 5      # the smallest height of the AIR 8 quotient tests


@pytest.fixture(scope="module")
def ctl():
    return [int(v) for v in rand_field(np.random.default_rng(41), (4,), edge=False)]


def test_models_agree_with_integers():
    rng = np.random.default_rng(1)
    words = rng.integers(0, 1 << 64, size=(200000, 2), dtype=np.uint64)
    pairs = [(int(a), int(b)) for a, b in words] + lo.edge_pairs()
    for a, b in pairs:
        r = lo.mul_model(a, b)
        assert 0 <= r < 1 << 64 and r % P == a * b % P, (hex(a), hex(b))
    for a, b in pairs[:20000] + lo.edge_pairs():
        cb = b % P
        for model, want in ((lo.add_model, a + cb), (lo.sub_model, a - cb)):
            r = model(a, cb)
            assert 0 <= r < 1 << 64 and r % P == want % P, (model.__name__, hex(a), hex(b))
        r = lo.mul7_model(a)
        assert 0 <= r < 1 << 64 and r % P == 7 * a % P, hex(a)
        assert [v % P for v in lo.sbox_model(a)] == [pow(a, e, P) for e in (2, 4, 3, 7)], hex(a)
    assert lo.mul_model(P, 12345) == P       # a non-canonical zero


def test_pair_generators_reach_the_upper_representative():
    rng = np.random.default_rng(2)
    for gen, bound in ((lo.generic_small_pairs, 1 << 16), (lo.beta_small_pairs, 16)):
        pairs = gen(rng, 20000)
        assert all(0 < a < P and 0 < b < P and 0 < a * b % P < bound for a, b in pairs)
        upper = sum(lo.mul_model(a, b) >= P for a, b in pairs)
        assert 10 * upper >= 9 * len(pairs), (gen.__name__, upper)
    # ... and a product of two small factors that are themselves in the upper representative does not stay there
    assert all(lo.mul_model(s + P, t + P) < P for s in range(1, 16) for t in range(1, 16))


def test_chunk_matrices_reach_every_level_on_both_sides(ctl):
    rng = np.random.default_rng(3)
    consts, trace, aux = lo.plonk_chunk_matrices(LOG_N, ctl, rng)
    rows = (1 << LOG_N) << 3
    assert consts.shape == (85, rows) and trace.shape == (135, rows) and aux.shape == (20, rows)
    assert all((m < np.uint64(P)).all() for m in (consts, trace, aux))
    count = lo.rows_with_upper_words(LOG_N, ctl, consts, trace, aux)
    assert set(count) == {(s, lv) for s in ("num", "den") for lv in lo.LEVELS + (5,)}
    for key, n in count.items():
        assert 5 * n >= rows, (key, n, rows)
    # no term of a steered chain is zero
    xs, windows = lo.coset_points(LOG_N), 0
    for row in range(0, rows, 7):
        for u in range(lo.N_CHUNKS):
            w = [int(trace[8 * u + i, row]) for i in range(8)]
            sg = [int(consts[lo.CST_SIGMA + 8 * u + i, row]) for i in range(8)]
            cls, c = lo.chunk_class(row, u)
            pcol, ccol = lo.z_columns(u, c)
            if cls == lo.GENERIC or (cls in (lo.CLOSE_NUM, lo.WINDOW) and pcol is None):
                continue
            tree = lo.chunk_levels(u, ctl[2 * c], ctl[2 * c + 1], xs[row], w, sg,
                                   int(aux[pcol, row]) if pcol is not None else 0, int(aux[ccol, row]))
            assert all(v % P for side in ("num", "den") for v in tree[side][1])
            if cls == lo.WINDOW:
                windows += 1
                g_num, g_den = tree["num"][5][0], tree["den"][5][0]
                assert all(v >= P for v in tree["den"][3]) and 0 < g_den < 1 << 12 <= g_num - P < 1 << 16, (row, u)
                # ... where the canonical subtraction, given these words as they are, is off by 2^32 - 1
                assert (g_den + (P - g_num)) % (1 << 64) % P == (g_den - g_num + (1 << 32) - 1) % P
            else:
                side, level = {lo.CLOSE_NUM: ("num", 5), lo.CLOSE_DEN: ("den", 5)}.get(
                    cls, ("den", cls + 1) if cls < lo.NUM_L1 else ("num", cls - 3))
                assert any(v >= P for v in tree[side][level]), (row, u, cls)
    assert windows >= 20


def test_random_matrices_do_not(ctl):
    """what the existing quotient tests run on: not one upper representative past the first level"""
    rng = np.random.default_rng(4)
    consts, trace, aux = rand_field(rng, (85, 256)), rand_field(rng, (135, 256)), rand_field(rng, (20, 256))
    count = lo.rows_with_upper_words(LOG_N, ctl, consts, trace, aux)
    assert all(count[(s, lv)] == 0 for s in ("num", "den") for lv in (2, 3, 4, 5))


def test_hash_matrices_reach_every_round(ctl):
    rng = np.random.default_rng(5)
    consts, trace, aux = lo.plonk_hash_matrices(LOG_N, ctl, rng)
    rows = trace.shape[1]
    assert all((m < np.uint64(P)).all() for m in (consts, trace, aux))
    assert {int(v) for v in consts[lo.CST_HASH, 0:rows:3]} >= {0, 1} and len({int(v) for v in consts[lo.CST_HASH]}) > 3
    assert {int(v) for v in trace[lo.H_SWAP, 0:rows:3]} == {0, 1}
    upper_out, upper_x2_only = set(), set()
    for row in range(rows):
        if row % 3 == 2:
            continue
        if int(trace[lo.H_SWAP, row]) in (0, 1):     # the swap constraints hold on the steered rows
            s = int(trace[lo.H_SWAP, row])
            for i in range(4):
                d = (int(trace[lo.H_IN + 4 + i, row]) - int(trace[lo.H_IN + i, row])) % P
                assert int(trace[lo.H_DELTA + i, row]) == s * d % P
        for rnd, xs in enumerate(lo.hash_row_sbox_inputs(trace, row)):
            assert len(xs) == (12 if lo.is_full(rnd) else 1)
            forms = [lo.sbox_model(x) for x in xs]
            if all(f[3] >= P for f in forms):
                upper_out.add(rnd)
            if all(f[0] >= P and f[1] < P for f in forms):
                upper_x2_only.add(rnd)
    assert upper_out == set(range(30)) and upper_x2_only == set(range(30))


def test_integer_poseidon_matches_the_oracle_and_inverts(oracle):
    rng = np.random.default_rng(6)
    states = rand_field(rng, (24, 12))
    want = oracle.poseidon(states)
    for s, w in zip(states, want):
        got = lo.permute(s)
        assert got == [int(v) for v in w]
        assert lo.inverse(got) == [int(v) for v in s]
    assert [sum(a * b for a, b in zip(row, col)) % P for row in lo.MDS for col in zip(*lo.MDS_INV)] == \
        [1 if i == j else 0 for i in range(12) for j in range(12)]
    assert 7 * lo.SBOX_INV_EXP % (P - 1) == 1


def test_backsolved_states_have_the_small_words_they_claim():
    rng = np.random.default_rng(7)
    for rnd in range(30):
        words = range(12) if lo.is_full(rnd) else range(1)
        s = lo.state_with_small_sbox_outputs(rnd, rng)
        pre, post, _ = lo.forward_rounds(s)
        assert all(0 <= v < P for v in s) and all(0 < post[rnd][i] < 1 << 16 for i in words)
        assert all(lo.sbox_model(pre[rnd][i])[3] >= P for i in words)
        s = lo.state_with_small_squares(rnd, rng)
        pre, post, _ = lo.forward_rounds(s)
        assert all(0 < pre[rnd][i] ** 2 % P < 1 << 16 for i in words)
        forms = [lo.sbox_model(pre[rnd][i]) for i in words]
        assert all(f[0] >= P and f[1] < P for f in forms)


def test_fri_stage0_products_are_small():
    rng = np.random.default_rng(8)
    m = 32
    vals = lo.fri_stage0_small(rand_field(rng, (m, 2)), rng)
    w16_inv = lo.inv(pow(7, (P - 1) // 16, P))
    upper = total = 0
    for g in range(m // 16):
        for j in range(8):
            for comp in range(2):
                d = (int(vals[g + j * (m // 16), comp]) - int(vals[g + (j + 8) * (m // 16), comp])) % P
                w = pow(w16_inv, j, P)
                assert 0 < d * w % P < 1 << 16
                total += 1
                upper += lo.mul_model(d, w) >= P
    assert 10 * upper >= 7 * total     # j = 0 multiplies by one: those two of sixteen stay below p


def test_small_cells_come_from_both_halves():
    cells = lo.small_cells(np.random.default_rng(9), (16, 64))
    assert cells.dtype == np.uint64 and (cells < np.uint64(P)).all()
    assert {int(v) for v in cells.ravel()} >= set(lo.SMALL_ALPHABET)
    assert ((cells < 1 << 16) & (cells > 2)).sum() > cells.size // 4
