// word256.cuh -- what the witness kernels of the shipped tables (arithmetic_div.hip, arithmetic_mod.hip) share: a
// 256-bit word in named registers, its 16-bit limbs by compile-time number, and a lane's view of its trace row.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace word256 {

// A 256-bit word as four named 64-bit registers, least significant first: no array, so nothing a lane could index at
// run time and the compiler could send to scratch.
struct U256 {
  uint64_t a, b, c, d;
};
__device__ __forceinline__ U256 sub256(const U256& x, const U256& y, uint32_t* borrow_out) {
  U256 r;
  r.a = x.a - y.a;
  uint32_t bw = x.a < y.a;
  uint64_t t = x.b - y.b;
  uint32_t b2 = (x.b < y.b) | (t < bw);
  r.b = t - bw;
  t = x.c - y.c;
  uint32_t b3 = (x.c < y.c) | (t < b2);
  r.c = t - b2;
  t = x.d - y.d;
  *borrow_out = (x.d < y.d) | (t < b3);
  r.d = t - b3;
  return r;
}
// limb K (16 bits) of a word, K a compile-time number
template <uint32_t K>
__device__ __forceinline__ uint32_t limb(const U256& w) {
  const uint64_t v = K < 4 ? w.a : K < 8 ? w.b : K < 12 ? w.c : w.d;
  return (uint32_t)(v >> (16 * (K & 3))) & 0xFFFFu;
}

struct Row {
  uint64_t* t;  // the trace at this lane's row: column c at t[c * n]
  uint64_t n;
  __device__ __forceinline__ void put(uint32_t col, uint64_t v) const { t[(uint64_t)col * n] = v; }
  // `count` bit columns from `col`: bit j of v at col + j
  __device__ __forceinline__ void put_bits(uint32_t col, uint32_t v, uint32_t count) const {
#pragma unroll 1
    for (uint32_t j = 0; j < count; j++) put(col + j, (v >> j) & 1u);
  }
};

}  // namespace word256
