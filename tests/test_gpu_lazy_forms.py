"""The lazily reduced field forms where they turn non-canonical.  gl::mul / mul_n / add / sub / mul7 and
poseidon::sbox return ANY 64-bit representative of a residue, and the kernels that use them (AIR 8's copy products and
Poseidon gate, the permutation in all its forms, the sponge and tree kernels, the FRI fold) promise in comments that
such a word passes through a canonicalising step before anything compares, stores or canonically adds it.  A broken
promise shows only when the word is in [p, 2^64), i.e. when the residue is below 2^32 - 1: on the uniformly random
operands of the other parity tests that is one value in 2^32.  Here the operands are built to get there
(tests/lazy_operands.py, held to its claims on the host by tests/test_lazy_operands.py), and every kernel is compared
with the oracle bit for bit."""
import numpy as np
import pytest

import lazy_operands as lo
from builtin_airs import AIRS, to_coset_major
from lazy_operands import P
from test_gpu_kernels import perm_form, test_merkle_commit_matches_oracle as _merkle_test  # noqa: F401 (perm_form: a fixture)
from util import bitrev_perm, coset_major_to_natural, rand_field, to_dev, to_host

pytestmark = pytest.mark.gpu

MUL_PLANES = {"mul": [0], "mul_n<4>": [1, 2, 3, 4], "mul_n<3>": [5, 6, 7]}
EDGE_CTL = [(1 << 32) - 1, P - 1, P - (1 << 32), 1 << 32]


def test_raw_planes_of_the_lazy_forms(bpg):
    """bp_debug_lazy_forms on 2^16 pairs -- generic-small, beta-small, every edge pair, uniform u64 for the rest: every
    plane congruent to the Python integer result AND the very word the transcription of the form predicts; on the two
    steered families every multiply form returns the upper representative for at least nine pairs in ten (printed per
    form: profiles/lazy_forms.txt)."""
    rng = np.random.default_rng(21)
    n_steer = 1 << 14
    fam = {"generic-small": lo.generic_small_pairs(rng, n_steer), "beta-small": lo.beta_small_pairs(rng, n_steer)}
    pairs = fam["generic-small"] + fam["beta-small"] + lo.edge_pairs()
    rest = rng.integers(0, 1 << 64, size=((1 << 16) - len(pairs), 2), dtype=np.uint64)
    pairs += [(int(a), int(b)) for a, b in rest]
    assert len(pairs) == 1 << 16
    av, bv = (np.array([p[k] for p in pairs], dtype=np.uint64) for k in (0, 1))
    out = to_host(bpg.ops.lazy_forms(to_dev(av), to_dev(bv)))
    assert out.shape == (12, 1 << 16)
    got = [[int(v) for v in row] for row in out]
    for i, (a, b) in enumerate(pairs):
        cb = b % P
        prod = lo.mul_model(a, b)
        assert prod % P == a * b % P
        for plane in range(8):
            assert got[plane][i] % P == a * b % P, (plane, hex(a), hex(b))
            assert got[plane][i] == prod, (plane, hex(a), hex(b), hex(got[plane][i]), hex(prod))
        for plane, want, model in ((8, a + cb, lo.add_model(a, cb)), (9, a - cb, lo.sub_model(a, cb)),
                                   (10, 7 * a, lo.mul7_model(a)), (11, pow(a, 7, P), lo.sbox_model(a)[3])):
            assert got[plane][i] % P == want % P, (plane, hex(a), hex(b))
            assert got[plane][i] == model, (plane, hex(a), hex(b), hex(got[plane][i]), hex(model))
    for k, name in enumerate(fam):
        sl = slice(k * n_steer, (k + 1) * n_steer)
        predicted = sum(lo.mul_model(a, b) >= P for a, b in fam[name])
        for form, planes in MUL_PLANES.items():
            for plane in planes:
                upper = int((out[plane, sl] >= np.uint64(P)).sum())
                print("lazy_forms %-13s %-8s plane %d: upper representative in %d of %d pairs (transcription: %d)"
                      % (name, form, plane, upper, n_steer, predicted))
                assert 10 * upper >= 9 * n_steer, (name, form, plane, upper)


def plonk_quotient(bpg, oracle, log_n, mats, ctl, alphas, loaded):
    consts, trace, aux = mats
    want = oracle.quotient_values(oracle.plonk_cfg(log_n), consts, trace, aux, np.array(ctl, dtype=np.uint64), alphas[0], alphas[1])
    with bpg.ops.tuned(assume_loaded=loaded):
        got = bpg.ops.quotient_eval(bpg.ops.stark_cfg(log_n, 135, n_const=85, deg_pow=3, rate_bits=3),
                                    to_dev(to_coset_major(trace, log_n, 3)), to_dev(to_coset_major(aux, log_n, 3)),
                                    to_dev(to_coset_major(consts, log_n, 3)), ctl, alphas, air_id=8)
    return to_host(got), to_coset_major(want, log_n, 3)


@pytest.fixture(scope="module", params=["generic", "edge"])
def plonk_case(request):
    """(ctl, alphas, the chunk matrices, the hash matrices) for one set of challenges, built once"""
    rng = np.random.default_rng(31 if request.param == "generic" else 32)
    ctl = [int(v) for v in rand_field(rng, (4,), edge=False)] if request.param == "generic" else EDGE_CTL
    alphas = rand_field(rng, (2,), edge=False)
    return ctl, alphas, lo.plonk_chunk_matrices(5, ctl, rng), lo.plonk_hash_matrices(5, ctl, rng)


@pytest.mark.parametrize("loaded", [0, 1])
def test_plonk_chunk_units_on_steered_products(bpg, oracle, plonk_case, loaded):
    """AIR 8, units 0..9 (air.hpp eval_chunk_unit): every level of the copy-product tree -- beta sigma, the terms, the
    pairs, the halves, the products, the closing products with Z -- runs through upper representatives on (nearly) every
    row, numerator and denominator side (tests/test_lazy_operands.py counts them), and on three rows in four the closing
    subtraction meets the one pair of words it would get wrong if the closing F::mul4 left them unreduced (lazy_operands:
    "window"; with that mul4 made lazy 193 of 256 rows differ, on random matrices none); spread and one-pass form"""
    ctl, alphas, chunk, _ = plonk_case
    got, want = plonk_quotient(bpg, oracle, 5, chunk, ctl, alphas, loaded)
    bad = np.nonzero((got != want).any(axis=0))[0]
    assert bad.size == 0, "%d of %d rows differ, the first at coset-major position %d" % (bad.size, got.shape[1], bad[0])


@pytest.mark.parametrize("loaded", [0, 1])
def test_plonk_poseidon_gate_on_steered_sboxes(bpg, oracle, plonk_case, loaded):
    """AIR 8, unit 10 (eval_hash_unit, the pass of its own): rows whose S-box inputs in every round are 7th roots, or
    square roots, of small numbers; q_hash 1 / 0 / generic, the swap wire 0 / 1"""
    ctl, alphas, _, hashm = plonk_case
    got, want = plonk_quotient(bpg, oracle, 5, hashm, ctl, alphas, loaded)
    bad = np.nonzero((got != want).any(axis=0))[0]
    assert bad.size == 0, "%d of %d rows differ, the first at coset-major position %d" % (bad.size, got.shape[1], bad[0])


@pytest.mark.parametrize("air_id", [0] + sorted(AIRS))
def test_canonical_policy_airs_on_small_cells(bpg, oracle, air_id):
    """AIR 0..7 evaluate with the canonical policy (Ops::add / sub / mul): the comparison of their K5 tests at the
    smallest height each runs, on cells from {0, 1, 2, p-1, p-2, 2^32-1, 2^32, p-2^32, 2^16-1} and limbs below 2^16,
    where differences and products are small or wrap -- the guard that they still do"""
    rng = np.random.default_rng(50 + air_id)
    if air_id == 0:
        log_n, n_cols, n_aux = 6, 16, 2
    else:
        log_n, n_cols, n_aux = min(AIRS[air_id].k5_log_n), AIRS[air_id].n_cols, AIRS[air_id].n_aux
    rows = (1 << log_n) << 1
    trace, aux = lo.small_cells(rng, (n_cols, rows)), lo.small_cells(rng, (n_aux, rows))
    ctl, alphas = rand_field(rng, (4,)), rand_field(rng, (2,))
    want = oracle.quotient_values(oracle.make_cfg(log_n, n_cols, air_id=air_id), None, trace, aux, ctl, alphas[0], alphas[1])
    got = bpg.ops.quotient_eval(bpg.ops.stark_cfg(log_n, n_cols), to_dev(to_coset_major(trace, log_n)),
                                to_dev(to_coset_major(aux, log_n)), None, ctl, alphas, air_id=air_id)
    assert (to_coset_major(want, log_n) == to_host(got)).all()


@pytest.fixture(scope="module")
def backsolved(oracle):
    """the 30 + 30 input states whose round-r S-boxes see small outputs / small squares, and their images"""
    rng = np.random.default_rng(61)
    states = [lo.state_with_small_sbox_outputs(r, rng) for r in range(30)]
    states += [lo.state_with_small_squares(r, rng) for r in range(30)]
    states = np.array(states, dtype=np.uint64)
    pad = rand_field(rng, (8, 12))
    return states, oracle.poseidon(states), pad, oracle.poseidon(pad)


def test_permutation_on_backsolved_states(bpg, backsolved, perm_form):
    """Every form of the batch permutation on states that reach, in one chosen round each, S-box outputs (or squares)
    in the upper representative: the matrix-core forms hand the bytes of that word to the MFMA.  Batches of 65 (all of
    them), of 17 and of 1."""
    states, want, pad, want_pad = backsolved
    batch, wb = np.concatenate([states, pad[:5]]), np.concatenate([want, want_pad[:5]])
    assert batch.shape == (65, 12)
    assert (to_host(bpg.ops.poseidon_perm_batch_(to_dev(batch))) == wb).all()
    for i0 in range(0, 60, 15):
        b17, w17 = np.concatenate([states[i0:i0 + 15], pad[5:7]]), np.concatenate([want[i0:i0 + 15], want_pad[5:7]])
        assert b17.shape == (17, 12)
        assert (to_host(bpg.ops.poseidon_perm_batch_(to_dev(b17))) == w17).all(), i0
    for i in range(60):
        assert (to_host(bpg.ops.poseidon_perm_batch_(to_dev(states[i:i + 1]))) == want[i:i + 1]).all(), i


MERKLE_FORMS = next(m.args[1] for m in _merkle_test.pytestmark if m.args[0] == "quad")


@pytest.fixture(scope="module")
def sponge_rows():
    """32 rows x 17 words: the first eight words of each row make round 0's S-box inputs of the rate words 7th roots
    (even rows) or square roots (odd rows) of small numbers -- root - rc_0; the capacity starts at zero"""
    rng = np.random.default_rng(71)
    rows = rand_field(rng, (17, 32))
    for r in range(32):
        pick = lo.seventh_root_of_small if r % 2 == 0 else lo.root_of_small_square
        for i in range(8):
            rows[i, r] = (pick(rng) - lo.RC[i]) % P
    return rows


@pytest.mark.parametrize("form", MERKLE_FORMS)
def test_merkle_commit_on_backsolved_rows(bpg, oracle, sponge_rows, form):
    """bp_merkle_commit in every form of test_merkle_commit_matches_oracle on rows whose first absorb runs its S-boxes
    through upper representatives; 5 / 8 / 9 columns around the first rate boundary, 16 / 17 around the second"""
    log_n, rate_bits = 4, 1
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
    idx = coset_major_to_natural(log_n, rate_bits)
    for n_cols in (5, 8, 9, 16, 17):
        lde_cm = np.ascontiguousarray(sponge_rows[:n_cols])
        lde_nat = np.ascontiguousarray(lde_cm[:, idx])
        for cap_h in (0, 2):
            want_dig, want_cap = oracle.merkle_commit(lde_nat, cap_h, bitrev_rows=True)
            with bpg.ops.tuned(**knobs):
                dig = to_host(bpg.ops.merkle_commit(to_dev(lde_cm), log_n, rate_bits, cap_h))
            assert (dig == want_dig).all(), (n_cols, cap_h)
            assert (dig[-(1 << cap_h):] == want_cap).all(), (n_cols, cap_h)


@pytest.mark.parametrize("log_nl,rate_bits", [(4, 1), (5, 3)])
def test_fri_fold_on_small_stage0_products(bpg, oracle, log_nl, rate_bits):
    """test_fri_fold_matches_oracle's comparison with v_(j+8) = v_j - s w_16^j: each of the fold's first-stage products
    d w has a residue below 2^16, in both components, and leaves gl::mul_n in the upper representative"""
    rng = np.random.default_rng(80 + log_nl)
    log_m = log_nl + rate_bits
    vals = lo.fri_stage0_small(rand_field(rng, (1 << log_m, 2)), rng)
    beta = rand_field(rng, (2,), edge=False)
    shift = int(pow(7, 16, P))
    br = bitrev_perm(log_m)
    want_br = oracle.fri_fold(vals[br], 4, shift, beta)
    cm = np.empty_like(vals)
    cm[coset_major_to_natural(log_nl, rate_bits)] = vals
    got = to_host(bpg.ops.fri_fold(to_dev(cm), log_nl, rate_bits, shift, beta))
    nat = got[coset_major_to_natural(log_nl - 4, rate_bits)]
    assert (nat[bitrev_perm(log_m - 4)] == want_br).all()
