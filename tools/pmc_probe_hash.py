"""One Merkle commitment of a 2^20 x 64 table (2^21 rows x 8 permutations) with the matrix-core kernels and one with one
lane per state, for `rocprofv3 --pmc ...` passes over SQ counters (how VALU and MFMA issue share a SIMD)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import proof_protocol_decoder_amd as bpg
log_n, cols, r = 20, 64, 1
lde = torch.randint(0, 2**62, (cols, 1 << (log_n + r)), dtype=torch.int64, device="cuda")
# matrix cores + three groups (all 22 partial rounds) / per round; one lane per state
for knobs in ({}, {"poseidon_grouped": 0}, {"poseidon_mx": 0}):
    with bpg.ops.tuned(**knobs):
        bpg.ops.merkle_commit(lde, log_n, r, 4)
        torch.cuda.synchronize()
print("perms per commit:", (1 << (log_n + r)) * 9)
