"""AIR 1 (Keccak-f[1600], csrc/air.hpp) on the GPU against the oracle's independent statement of it
(oracle/keccak_air.c): the witness generator, K5 alone through bp_quotient_eval, and whole table proofs byte for byte
-- BASELINE configs[3] ("wide Keccak-f STARK trace, 2^20 rows") is the last one.  The first four tests are
builtin_airs.gpu_tests, the same for all seven AIRs, over this AIR's record (its shapes, seeds and spot checks, with a
note on why those heights)."""
import hashlib
import json
import os

import numpy as np
import pytest

import builtin_airs as ba

pytestmark, test_witness_matches_oracle, test_quotient_eval_matches_oracle, test_table_proof_bit_exact, \
    _wrong_shapes_are_refused = ba.gpu_tests(ba.keccak)


def test_wrong_shapes_for_the_air_are_refused(bpg):
    from proof_protocol_decoder_amd._lib import BpgError
    _wrong_shapes_are_refused(bpg)
    with pytest.raises(BpgError, match="unknown air_id"):
        bpg.ops.stark_prove_air(9, bpg.ops.stark_cfg(6, 16), 1)


@pytest.mark.parametrize("log_n", [17, 20])
def test_keccak_f_trace_at_baseline_size_matches_the_oracle(bpg, oracle, log_n):
    """BASELINE configs[3] as a REAL Keccak-f trace: 2^20 rows (43690 permutations and a cut one) x 2431 columns,
    rate 2, standard_fast_config, one GPU.  The oracle's proof of the same table was made once on the GPU box's host
    cores (tools/gen_cfg4_golden.py 20 keccak_f) and its sha256 is committed; the GPU proof must have it, verify
    under both verifiers, and stop verifying after a bit flip.  At this height the quotient is ONE pass: 8192
    workgroups, the alpha fold never leaves the registers."""
    import torch
    free, _ = torch.cuda.mem_get_info()
    need = 8 * (1 << log_n) * 2431 * 6.5
    if free < need:
        pytest.skip("needs ~%.0f GB of free device memory, %.0f GB free" % (need / 1e9, free / 1e9))
    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hotpath_golden.json")))["tables"]
    key = "logn%d_keccak_f" % log_n
    if key not in gold:
        pytest.skip("no oracle digest for %s yet (tools/gen_cfg4_golden.py %d keccak_f)" % (key, log_n))
    pc = bpg.ops.stark_cfg(log_n, 2431)
    try:
        got = bpg.ops.stark_prove_air(1, pc, ba.keccak.gpu_seed)
    finally:
        bpg.lib().bp_release_cached_memory()
    want = gold[key]
    assert got.size == want["n_words"] and [int(x) for x in got[:6]] == want["head"] and [int(x) for x in got[-2:]] == want["tail"]
    assert hashlib.sha256(np.ascontiguousarray(got, dtype="<u8").tobytes()).hexdigest() == want["sha256"]
    assert ba.product_verify(pc, 1, got) == 0
    cfg = oracle.make_cfg(log_n, 2431, air_id=1)
    ch = oracle.PyChallenger()
    ch.observe(got[16:16 + 64])
    ctl = np.array([ch.challenge() for _ in range(4)], dtype=np.uint64)
    assert oracle.stark_verify(cfg, got, ctl, ch, None) == 0
    bad = got.copy()
    bad[got.size // 3] ^= np.uint64(1 << 17)
    assert ba.product_verify(pc, 1, bad) != 0
