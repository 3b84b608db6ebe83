// Host check of csrc/plonk_hash_fold.hpp, a program of its own so that it can run under the host sanitizers:
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -I proof_protocol_decoder_amd/csrc -I include -o fold_check tools/plonk_hash_fold_host_check.cpp && ./fold_check
// It touches no device.  For a set of alphas it evaluates the constant table (hash_fold_table) the way
// alpha_table_kernel's three workgroups do -- every workgroup its pieces of at most four alpha powers against constant
// coefficients, an output per lane adding its pieces -- and compares the block with the one the recurrences give (hash_fold_block_host); it also checks every index the table
// holds against the bounds the kernel relies on.
#include <cstdio>
#include <vector>
#include "plonk_hash_fold.hpp"

namespace pk = bpg::air::plonk;

int main() {
  const uint32_t T = pk::N_CONSTRAINTS + bpg::air::ctl::PLONK_N_CONSTRAINTS, e0 = T - 1 - pk::G4, B = pk::HASH_FOLD_BLOCKS;
  if (T < pk::HASH_FOLD_T_MIN || T > pk::HASH_FOLD_T_MAX) return std::printf("FAIL: T = %u\n", T), 1;
  const std::vector<uint64_t> tab = pk::hash_fold_table();
  if (tab.size() != pk::HASH_FOLD_COEF0 + 256 * B * pk::HASH_FOLD_PIECE_TERMS) return std::printf("FAIL: no table\n"), 1;
  uint32_t pieces = 0, outputs = 0, most = 0;
  for (uint32_t l = 0; l < 256 * B; l++) {
    const uint64_t piece = tab[l];
    const uint32_t terms = (uint32_t)piece & 0xff, k0 = (uint32_t)(piece >> 8) & 0xff;
    if (!terms) continue;
    pieces++;
    if (terms > pk::HASH_FOLD_PIECE_TERMS || k0 + terms > pk::HASH_FOLD_PAIRS)
      return std::printf("FAIL: piece %u out of bounds\n", l), 1;
  }
  std::vector<int> seen(pk::HASH_FOLD_OUTPUTS, 0);
  for (uint32_t l = 0; l < 256 * B; l++) {
    const uint64_t o = tab[256 * B + l];
    const uint32_t n = (uint32_t)o & 0xff, first = (uint32_t)(o >> 8) & 0xff, slot = (uint32_t)(o >> 16);
    if (!n) continue;
    outputs++;
    most = n > most ? n : most;
    if (first + n > 256 || slot >= pk::HASH_FOLD_OUTPUTS || seen[slot]++) return std::printf("FAIL: output lane %u out of bounds\n", l), 1;
  }
  if (outputs != pk::HASH_FOLD_OUTPUTS) return std::printf("FAIL: %u outputs\n", outputs), 1;
  const uint64_t alphas[] = {0, 1, gl::P - 1, 0xFFFFFFFFULL, gl::P - (1ULL << 32), 0x317017a6205738d1ULL, 0x6018366cf658f7a7ULL, 7};
  for (uint64_t a : alphas) {
    uint64_t want[pk::HASH_FOLD_WORDS], got[pk::HASH_FOLD_WORDS] = {};
    pk::hash_fold_block_host(T, a, a, want);
    uint64_t pw[256];
    for (uint32_t l = 0; l < 256; l++) pw[l] = l < T ? gl::pow(a, l) : 0;
    for (uint32_t b = 0; b < B; b++) {  // a workgroup of alpha_table_kernel
      uint64_t part[256];
      for (uint32_t l = 0; l < 256; l++) {
        const uint64_t piece = tab[256 * b + l];
        const uint32_t terms = (uint32_t)piece & 0xff, k0 = (uint32_t)(piece >> 8) & 0xff;
        const uint64_t* coef = tab.data() + pk::HASH_FOLD_COEF0 + pk::HASH_FOLD_PIECE_TERMS * (256 * b + l);
        uint64_t acc = 0;
        for (uint32_t i = 0; i < terms; i++) acc = gl::addc(acc, gl::mulc(coef[i], pw[e0 - k0 - i]));
        part[l] = acc;
      }
      for (uint32_t l = 0; l < 256; l++) {
        const uint64_t o = tab[256 * B + 256 * b + l];
        const uint32_t n = (uint32_t)o & 0xff, first = (uint32_t)(o >> 8) & 0xff, slot = (uint32_t)(o >> 16);
        if (!n) continue;
        uint64_t sum = 0;
        for (uint32_t i = 0; i < n; i++) sum = gl::addc(sum, part[first + i]);
        for (uint32_t j = 0; j < 2; j++) got[2 * slot + j] = slot < pk::HASH_FOLD_PAIRS ? gl::negc(sum) : sum;
      }
    }
    for (uint32_t i = 0; i < pk::HASH_FOLD_WORDS; i++)
      if (got[i] != want[i]) return std::printf("FAIL: alpha %#llx word %u\n", (unsigned long long)a, i), 1;
  }
  std::printf("ok: %u pieces in %u workgroups (an output adds at most %u), %zu table words, %zu alphas\n", pieces, B, most, tab.size(),
              sizeof(alphas) / sizeof(alphas[0]));
  return 0;
}
