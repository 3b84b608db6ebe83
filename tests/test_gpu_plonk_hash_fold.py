"""AIR 8's quotient with the Poseidon gate folded in transposed form (quotient_plonk_hash_kernel: 118 S-boxes and the
weights of csrc/plonk_hash_fold.hpp instead of thirty MDS layers a row) against the oracle, bit for bit on every row of
the smallest recursion-shaped quotient (2^5 rows, rate 8), at the alpha pairs where the weights degenerate -- alpha = 0
leaves one non-zero power, 1 and -1 make all of them +-1 -- or sit at the edges of the 32-bit halves, with the selector
column 0, 1 and generic, in the spread and the one-pass form of the chunk units."""
import numpy as np
import pytest

import os
import sys

import lazy_operands as lo
from builtin_airs import to_coset_major
from util import P, rand_field, to_dev, to_host

pytestmark = pytest.mark.gpu

LOG_N = 5
ALPHA_PAIRS = {"0,1": (0, 1), "1,-1": (1, P - 1), "2^32-1,-2^32": ((1 << 32) - 1, P - (1 << 32)),
               "random": tuple(int(v) for v in rand_field(np.random.default_rng(41), (2,), edge=False))}
MATRICES = ["q_hash=0", "q_hash=1", "generic", "steered", "swapped"]
# the gate's layout from the model, which tests/test_plonk_hash_fold_model.py holds to csrc/air.hpp
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from plonk_hash_fold_model import CST_HASH, H_DELTA, H_IN, H_SWAP, N_AUX, N_COLS, N_CONST  # noqa: E402


def _matrices(kind):
    """(ctl, consts [85], trace [135], aux [20]) over the 256 LDE rows"""
    rng = np.random.default_rng(100 + MATRICES.index(kind))
    rows = (1 << LOG_N) << 3
    ctl = [int(v) for v in rand_field(rng, (4,), edge=False)]
    if kind == "steered":   # every S-box input a 7th or a square root of a small number: non-canonical S-box outputs
        return (ctl,) + tuple(lo.plonk_hash_matrices(LOG_N, ctl, rng))
    consts, trace, aux = rand_field(rng, (N_CONST, rows)), rand_field(rng, (N_COLS, rows)), rand_field(rng, (N_AUX, rows))
    if kind.startswith("q_hash="):
        consts[CST_HASH, :] = int(kind[-1])
    if kind == "swapped":   # the swap wire 1 and delta = in[4 + i] - in[i] != 0 on every row: the swap constraints hold
        trace[H_SWAP, :] = 1
        for i in range(4):
            same = trace[H_IN + 4 + i] == trace[H_IN + i]
            trace[H_IN + 4 + i, same] = (trace[H_IN + i, same] + np.uint64(1)) % np.uint64(P)
            trace[H_DELTA + i] = [(int(b) - int(a)) % P for a, b in zip(trace[H_IN + i], trace[H_IN + 4 + i])]
        assert (trace[H_DELTA:H_DELTA + 4] != 0).all()
    return ctl, consts, trace, aux


_CASES, _WANT = {}, {}


def _case(kind):
    if kind not in _CASES:
        ctl, consts, trace, aux = _matrices(kind)
        _CASES[kind] = (ctl, consts, trace, aux, [to_dev(to_coset_major(m, LOG_N, 3)) for m in (trace, aux, consts)])
    return _CASES[kind]


def _want(oracle, kind, pair):
    """the oracle's quotient values, once per matrices and alpha pair (shared by the two forms)"""
    if (kind, pair) not in _WANT:
        ctl, consts, trace, aux, _ = _case(kind)
        a0, a1 = ALPHA_PAIRS[pair]
        want = oracle.quotient_values(oracle.plonk_cfg(LOG_N), consts, trace, aux, np.array(ctl, dtype=np.uint64), a0, a1)
        _WANT[kind, pair] = to_coset_major(want, LOG_N, 3)
    return _WANT[kind, pair]


@pytest.mark.parametrize("loaded", [0, 1])
@pytest.mark.parametrize("pair", list(ALPHA_PAIRS))
@pytest.mark.parametrize("kind", MATRICES)
def test_plonk_quotient_with_the_transposed_gate(bpg, oracle, kind, pair, loaded):
    ctl, _, _, _, (d_trace, d_aux, d_consts) = _case(kind)
    want = _want(oracle, kind, pair)
    with bpg.ops.tuned(assume_loaded=loaded):
        got = to_host(bpg.ops.quotient_eval(bpg.ops.stark_cfg(LOG_N, N_COLS, n_const=N_CONST, deg_pow=3, rate_bits=3),
                                            d_trace, d_aux, d_consts, ctl, ALPHA_PAIRS[pair], air_id=8))
    assert got.shape == want.shape == (2, (1 << LOG_N) << 3)
    bad = np.nonzero((got != want).any(axis=0))[0]
    assert bad.size == 0, "%d of %d rows differ, the first at coset-major position %d" % (bad.size, got.shape[1], bad[0])

