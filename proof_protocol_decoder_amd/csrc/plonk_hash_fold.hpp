// plonk_hash_fold.hpp -- AIR 8's Poseidon gate with its MDS layers moved from the data onto the fold's weights.
//
// plonk::eval_hash_unit (air.hpp) is the gate: 118 constraints  d_k = wire_k - (an affine function of S-box outputs),
// constraint G4 + k for k < 118, and every S-box input is a wire (round 0's: in +- delta + rc_0).  The quotient uses
// only  sum_k A_k d_k  per challenge, A_k = alpha^(T - 1 - G4 - k), so
//     sum_k A_k d_k  =  sum_k A_k wire_k  -  sum_s C_s sigma_s  -  K
// where C (118 words) and K depend on alpha, the MDS matrix and the round constants alone: the same for every row of a
// quotient.  A row then costs 118 S-boxes and 2 x 118 dot terms and carries no state through thirty layers
// (quotient_plonk_hash_kernel, stark_kernels.hip).  tools/plonk_hash_fold_model.py is the model: both folds over
// Python integers, and the weights the tests hold these to.
//
// PAIRS.  Pair p < 106: the wire of constraint G4 + p (columns H_FULL1 .. H_SWAP - 1) with the S-box output of that
// very wire; pair 106 + i: output wire i (constraint G4 + 106 + i) with round 0's S-box output i.  The wire's weight is
// the alpha power of its constraint, read from the alpha table as every other constraint's; the S-box outputs' weights
// are the block behind the coset constants of QuotArgs::apow: [118][2] = {-C_0[p], -C_1[p]} (the two challenges), then
// K_0, K_1 (plonk::HASH_FOLD_WORDS words).
//
// WHERE THE WEIGHTS ARE MADE.  C and K are linear in (A_0 .. A_117), and each of them reads a run of consecutive A's --
// twelve for a full round's S-box output, up to 34 (the partial rounds' and round 26's constraints) for the S-box outputs
// the partial section hangs on, 106 for K.  hash_fold_table() cuts those runs into pieces of at most four terms and
// deals the outputs, whole, to HASH_FOLD_BLOCKS workgroups of alpha_table_kernel: each makes the T <= 256 alpha powers
// (a lane each, as the kernel always did; workgroup 0 also writes them out), then a lane per piece multiplies its
// powers by constant coefficients and a lane per output adds its pieces.  A lane's work stays within a few products of
// the power it made anyway.  The coefficients come from hash_fold_weights -- the recurrences, stated once -- applied to
// the unit vectors, once per device and process.
#pragma once
#include <cstdint>
#include <vector>
#include "air.hpp"
#include "gl.hpp"

namespace bpg {
namespace air {
namespace plonk {

// the pair of sigma^(r)_i (full rounds r = 0..3, 26..29) and of sigma_r (partial rounds r = 4..25)
inline uint32_t hash_fold_pair_full(uint32_t r, uint32_t i) {
  return r == 0 ? 106 + i : r <= 3 ? 12 * (r - 1) + i : 58 + 12 * (r - 26) + i;
}
inline uint32_t hash_fold_pair_part(uint32_t r) { return 36 + (r - 4); }

// A[k]: the weight of constraint G4 + k.  C[p]: the weight of pair p's S-box output; K: the constant.
//   full rounds r = 1..3, 27..29 and the output block (weights w = their twelve A's):  C[sigma^(r-1)] = M^T w,
//     K += w . rc_r  (the output block has no constants);
//   the partial section backwards: g = (round 26's A's), K += g . rc_26; for r = 25 .. 4: h = M^T g, C[sigma_r] = h[0],
//     g = h with g[0] = A of round r's constraint, K += g . rc_r; at the end C[sigma^(3)] = M^T g.
inline void hash_fold_weights(const uint64_t (&A)[HASH_FOLD_PAIRS], uint64_t (&C)[HASH_FOLD_PAIRS], uint64_t& K) {
  auto mds_t = [](const uint64_t (&g)[12], uint64_t (&h)[12]) {
    for (uint32_t c = 0; c < 12; c++) {
      uint64_t acc = 0;
      for (uint32_t r = 0; r < 12; r++) acc = gl::addc(acc, gl::mulc(poseidon_mds_entry(r, c), g[r]));
      h[c] = acc;
    }
  };
  auto dot_rc = [](const uint64_t (&g)[12], uint32_t r) {
    uint64_t acc = 0;
    for (uint32_t i = 0; i < 12; i++) acc = gl::addc(acc, gl::mulc(g[i], poseidon_rc(12 * r + i)));
    return acc;
  };
  K = 0;
  uint64_t g[12], h[12];
  auto full = [&](uint32_t k0, int rc_round, uint32_t sigma_round) {
    for (uint32_t i = 0; i < 12; i++) g[i] = A[k0 + i];
    mds_t(g, h);
    for (uint32_t i = 0; i < 12; i++) C[hash_fold_pair_full(sigma_round, i)] = h[i];
    if (rc_round >= 0) K = gl::addc(K, dot_rc(g, (uint32_t)rc_round));
  };
  for (uint32_t r = 1; r <= 3; r++) full(12 * (r - 1), (int)r, r - 1);
  for (uint32_t r = 27; r <= 29; r++) full(58 + 12 * (r - 26), (int)r, r - 1);
  full(106, -1, 29);
  for (uint32_t i = 0; i < 12; i++) g[i] = A[58 + i];
  K = gl::addc(K, dot_rc(g, 26));
  for (uint32_t r = 25; r >= 4; r--) {
    mds_t(g, h);
    C[hash_fold_pair_part(r)] = h[0];
    for (uint32_t i = 0; i < 12; i++) g[i] = h[i];
    g[0] = A[hash_fold_pair_part(r)];
    K = gl::addc(K, dot_rc(g, r));
  }
  mds_t(g, h);
  for (uint32_t i = 0; i < 12; i++) C[hash_fold_pair_full(3, i)] = h[i];
}

// The block the device reads, made on the host: out[2 p + j] = -C_j[p], out[2 * 118 + j] = K_j, for the constraint list
// of T entries (A_k = alpha^(T - 1 - G4 - k)).  (What alpha_table_kernel writes; the debug entries and the tests
// compare the two.)
inline void hash_fold_block_host(uint32_t T, uint64_t alpha0, uint64_t alpha1, uint64_t (&out)[HASH_FOLD_WORDS]) {
  for (uint32_t j = 0; j < 2; j++) {
    uint64_t A[HASH_FOLD_PAIRS], C[HASH_FOLD_PAIRS], K;
    for (uint32_t p = 0; p < HASH_FOLD_PAIRS; p++) A[p] = gl::pow(j ? alpha1 : alpha0, T - 1 - G4 - p);
    hash_fold_weights(A, C, K);
    for (uint32_t p = 0; p < HASH_FOLD_PAIRS; p++) out[2 * p + j] = gl::negc(C[p]);
    out[2 * HASH_FOLD_PAIRS + j] = K;
  }
}

// The constant table of alpha_table_kernel's fold workgroups (u64 words), B = HASH_FOLD_BLOCKS workgroups of 256 lanes:
//   [0, 256 B)        a piece per lane of workgroup b = index / 256: terms | first A index << 8   (0 terms: an idle lane)
//   [256 B, 512 B)    an output per lane of the same workgroup: pieces | first piece (a lane of the workgroup) << 8 |
//                     slot << 16, slot = the pair whose C it is, or 118 for K   (0 pieces: an idle lane)
//   [512 B, 1536 B)   the coefficients: four words a lane, the piece's in the order of its A's (the rest 0) -- at a
//                     fixed place, so that no load of a lane waits for another
// Every piece of an output lies in the output's workgroup.
constexpr uint32_t HASH_FOLD_BLOCKS = 3, HASH_FOLD_OUTPUTS = HASH_FOLD_PAIRS + 1, HASH_FOLD_PIECE_TERMS = 4;
constexpr uint32_t HASH_FOLD_COEF0 = 2 * 256 * HASH_FOLD_BLOCKS;
constexpr uint32_t HASH_FOLD_T_MIN = G4 + HASH_FOLD_PAIRS, HASH_FOLD_T_MAX = 256;  // every power a lane of one workgroup, none negative
inline std::vector<uint64_t> hash_fold_table() {
  // column k of the linear map: the weights of the unit vector e_k
  std::vector<uint64_t> col((size_t)HASH_FOLD_PAIRS * HASH_FOLD_OUTPUTS);
  for (uint32_t k = 0; k < HASH_FOLD_PAIRS; k++) {
    uint64_t A[HASH_FOLD_PAIRS] = {}, C[HASH_FOLD_PAIRS], K;
    A[k] = 1;
    hash_fold_weights(A, C, K);
    for (uint32_t p = 0; p < HASH_FOLD_PAIRS; p++) col[(size_t)k * HASH_FOLD_OUTPUTS + p] = C[p];
    col[(size_t)k * HASH_FOLD_OUTPUTS + HASH_FOLD_PAIRS] = K;
  }
  std::vector<uint64_t> tab(HASH_FOLD_COEF0 + 256 * HASH_FOLD_BLOCKS * HASH_FOLD_PIECE_TERMS, 0);
  uint32_t block = 0, piece = 0, output = 0;  // the workgroup being filled, its next free piece and output lanes
  for (uint32_t o = 0; o < HASH_FOLD_OUTPUTS; o++) {
    uint32_t lo = HASH_FOLD_PAIRS, hi = 0;  // the run of A's the output reads
    for (uint32_t k = 0; k < HASH_FOLD_PAIRS; k++)
      if (col[(size_t)k * HASH_FOLD_OUTPUTS + o]) {
        if (lo == HASH_FOLD_PAIRS) lo = k;
        hi = k;
      }
    if (lo == HASH_FOLD_PAIRS) return {};  // (cannot happen: every S-box output is constrained)
    const uint32_t n = (hi - lo + HASH_FOLD_PIECE_TERMS) / HASH_FOLD_PIECE_TERMS;
    if (piece + n > 256) { block++; piece = output = 0; }
    if (block >= HASH_FOLD_BLOCKS || n > 255) return {};  // (cannot happen: 555 pieces)
    tab[256 * HASH_FOLD_BLOCKS + 256 * block + output++] = (uint64_t)n | (uint64_t)piece << 8 | (uint64_t)o << 16;
    for (uint32_t k0 = lo; k0 <= hi; k0 += HASH_FOLD_PIECE_TERMS) {
      const uint32_t k1 = k0 + HASH_FOLD_PIECE_TERMS - 1 < hi ? k0 + HASH_FOLD_PIECE_TERMS - 1 : hi;
      for (uint32_t k = k0; k <= k1; k++)
        tab[HASH_FOLD_COEF0 + HASH_FOLD_PIECE_TERMS * (256 * block + piece) + (k - k0)] = col[(size_t)k * HASH_FOLD_OUTPUTS + o];
      tab[256 * block + piece++] = (uint64_t)(k1 - k0 + 1) | (uint64_t)k0 << 8;
    }
  }
  return tab;
}

}  // namespace plonk
}  // namespace air
}  // namespace bpg
