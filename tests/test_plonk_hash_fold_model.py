"""AIR 8's Poseidon gate folded with the MDS layers on the weights (csrc/plonk_hash_fold.hpp, the device's
quotient_plonk_hash_kernel): the model's two folds against each other, and the weights the library makes against the
model's, at the alphas where powers collapse (0, 1, -1) or sit at the edge of the 32-bit halves."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import plonk_hash_fold_model as model  # noqa: E402

P = model.P
_rng = random.Random(20)
ALPHAS = [0, 1, P - 1, (1 << 32) - 1, P - (1 << 32)] + [_rng.randrange(P) for _ in range(3)]


def test_model_layout_is_the_headers():
    """the model's copies of the gate's layout against csrc/air.hpp, so that a moved column or index fails here"""
    import re
    text = open(os.path.join(ROOT, "proof_protocol_decoder_amd", "csrc", "air.hpp")).read()
    text = text[text.index("namespace plonk {"):]
    consts = dict((k, int(v)) for line in re.findall(r"constexpr uint32_t ([^;]+);", text)
                  for k, v in re.findall(r"(\w+) = (\d+)(?=,|$)", line))
    for name in ("H_IN", "H_OUT", "H_FULL1", "H_PART", "H_FULL2", "H_SWAP", "H_DELTA", "H_WIRES", "G4", "G5", "N_CONSTRAINTS",
                 "N_COLS", "N_CONST", "CST_HASH"):
        assert consts[name] == getattr(model, name), name
    assert consts["HASH_FOLD_PAIRS"] == model.N_PAIRS
    assert consts["PLONK_N_CONSTRAINTS"] == model.N_CTL_CONSTRAINTS and consts["PLONK_N_AUX"] == model.N_AUX
    from proof_protocol_decoder_amd import ops
    assert ops.PLONK_HASH_FOLD_WORDS == model.FOLD_WORDS == 2 * consts["HASH_FOLD_PAIRS"] + 2   # HASH_FOLD_WORDS of air.hpp


@pytest.mark.parametrize("alpha", ALPHAS, ids=hex)
def test_transposed_fold_is_the_direct_fold(alpha):
    """random wires, wires from the edge alphabet, and a row with the swap wire 1"""
    rng = random.Random(alpha & 0xFFFF)
    edge = [0, 1, P - 1, (1 << 32) - 1, 1 << 32, P - (1 << 32)]
    rows = [[rng.randrange(P) for _ in range(model.H_WIRES)] for _ in range(3)]
    rows.append([rng.choice(edge) for _ in range(model.H_WIRES)])
    swapped = [rng.randrange(P) for _ in range(model.H_WIRES)]
    swapped[model.H_SWAP] = 1
    rows.append(swapped)
    for w in rows:
        assert model.direct_fold(w, alpha) == model.transposed_fold(w, alpha)


def test_host_weights_are_the_models():
    """bp_debug_plonk_hash_fold_host (the recurrences of plonk_hash_fold.hpp, from which the device's constant table is
    made) against the model's pair table, every alpha of the set on either side of the pair"""
    import proof_protocol_decoder_amd as pkg
    pkg.lib()
    for k, a0 in enumerate(ALPHAS):
        a1 = ALPHAS[(k + 3) % len(ALPHAS)]
        got = pkg.ops.plonk_hash_fold_host((a0, a1))
        want = np.array(model.pair_table(a0, a1), dtype=np.uint64)
        assert got.shape == want.shape and (got == want).all(), (hex(a0), hex(a1), np.nonzero(got != want)[0][:8])


@pytest.mark.gpu
def test_device_weights_are_the_models(bpg):
    """bp_debug_plonk_hash_fold: the block alpha_table_kernel's three workgroups leave behind the coset constants (pieces
    of at most four alpha powers against constant coefficients, summed per output) against the model's"""
    from util import to_host
    for k, a0 in enumerate(ALPHAS):
        a1 = ALPHAS[(k + 3) % len(ALPHAS)]
        got = to_host(bpg.ops.plonk_hash_fold((a0, a1)))
        want = np.array(model.pair_table(a0, a1), dtype=np.uint64)
        assert got.shape == want.shape and (got == want).all(), (hex(a0), hex(a1), np.nonzero(got != want)[0][:8])
