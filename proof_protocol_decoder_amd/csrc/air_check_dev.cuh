// air_check_dev.cuh -- the device pieces of the trace checker's kernels (air_check.hip: the built-in AIRs;
// air_program.hip: registered programs): row i of the trace as air.hpp's row accessors read it, the consumer with the
// trace domain's selectors, and the bitmap write.
#pragma once
#include "air_check.hpp"
#include "gl.hpp"
#include "air.hpp"

namespace bpg {
namespace chk {

using bpg::CheckArgs;

struct CheckRow {  // row i of the trace (lanes = consecutive rows: coalesced), no auxiliary columns
  const uint64_t *trace, *cst_;
  uint64_t ts, cs, pos, pos_next;
  uint64_t xv;
  const uint64_t* pub_;
  __device__ __forceinline__ uint64_t x() const { return xv; }
  __device__ __forceinline__ uint64_t pub(uint32_t j) const { return pub_[j]; }
  __device__ __forceinline__ uint64_t loc(uint32_t c) const { return trace[(uint64_t)c * ts + pos]; }
  __device__ __forceinline__ uint64_t nxt(uint32_t c) const { return trace[(uint64_t)c * ts + pos_next]; }
  __device__ __forceinline__ uint64_t cst(uint32_t k) const { return cst_[(uint64_t)k * cs + pos]; }
  __device__ __forceinline__ uint64_t aux(uint32_t) const { return 0; }
  __device__ __forceinline__ uint64_t aux_nxt(uint32_t) const { return 0; }
};
struct CheckEmit {  // K5's consumer (stark_kernels.hip, DevEmit) with the trace domain's selectors as masks
  const uint64_t* apow;  // [2][T]
  uint32_t T;
  uint64_t m_tr, m_first, m_last;  // all ones where the selector is 1, else zero
  gl::DotAcc acc[4];
  uint64_t pend_v;
  uint32_t pend_e;
  bool has;
  __device__ __forceinline__ void push(uint32_t idx, uint64_t v) {
    if (idx >= T) return;  // a lookup share: not the AIR's own constraint
    const uint32_t e = T - 1 - idx;
    if (!has) {
      pend_v = v; pend_e = e; has = true;
      return;
    }
    const uint64_t a[4] = {pend_v, pend_v, v, v};
    const uint64_t w[4] = {apow[pend_e], apow[T + pend_e], apow[e], apow[T + e]};
    gl::dot_mad4(acc, a, w);
    has = false;
  }
  __device__ __forceinline__ void all(uint32_t idx, uint64_t v) { push(idx, v); }
  __device__ __forceinline__ void transition(uint32_t idx, uint64_t v) { push(idx, v & m_tr); }
  __device__ __forceinline__ void first(uint32_t idx, uint64_t v) { push(idx, v & m_first); }
  __device__ __forceinline__ void last(uint32_t idx, uint64_t v) { push(idx, v & m_last); }
  // the same four by a run-time (wave-uniform) kind, through one push: the program interpreter's (air_program.hpp)
  __device__ __forceinline__ void emit(uint32_t kind, uint32_t idx, uint64_t v) {
    push(idx, kind == 0 ? v : v & (kind == 1 ? m_tr : kind == 2 ? m_first : m_last));
  }
  __device__ __forceinline__ uint64_t result(int j) {
    if (has) {
      const uint64_t a[4] = {pend_v, pend_v, 0, 0};
      const uint64_t w[4] = {apow[pend_e], apow[T + pend_e], 0, 0};
      gl::dot_mad4(acc, a, w);
      has = false;
    }
    return gl::addc(gl::dot_reduce(acc[j]), gl::dot_reduce(acc[2 + j]));
  }
};
__device__ __forceinline__ CheckEmit check_emit(const CheckArgs& a, uint64_t pos) {
  const uint64_t last = ((uint64_t)1 << a.log_n) - 1;
  return CheckEmit{a.apow, a.T, pos != last ? ~0ull : 0ull, pos == 0 ? ~0ull : 0ull, pos == last ? ~0ull : 0ull,
                   {gl::dot_zero(), gl::dot_zero(), gl::dot_zero(), gl::dot_zero()}, 0, 0, false};
}
__device__ __forceinline__ CheckRow check_row(const CheckArgs& a, uint64_t pos, bool with_x) {
  const uint64_t n = (uint64_t)1 << a.log_n;
  return CheckRow{a.trace, a.consts, a.stride, n, pos, (pos + 1) & (n - 1),
                  with_x ? gl::pow(gl::root(a.log_n), pos) : 0, a.pub};
}
// The filter f and the tuple of product column `col` of a BUILT-IN table with a lookup side at row `pos` of its trace
// (column stride `stride`), the tuple compressed under two challenges in ONE pass over it: v_k = sum_j beta_k^j t_j
// (air::ctl::port_tuple, what air::ctl::product_term compresses under one).  Keccak-f's looked tuple is its 50 input limbs,
// which the prover carries in the auxiliary column h and which are read here from the trace 23 rows up (the permutation's
// first row), then its 50 output limbs; a row with no permutation above it exposes nothing.
template <uint32_t AIR>
__device__ __forceinline__ void builtin_port_keys(const uint64_t* trace, uint64_t stride, uint64_t n, uint64_t pos, uint32_t col,
                                                  uint64_t beta0, uint64_t beta1, uint64_t* f, uint64_t* v0, uint64_t* v1) {
  namespace ctl = bpg::air::ctl;
  const CheckRow row{trace, nullptr, stride, 0, pos, (pos + 1) & (n - 1), 0, nullptr};
  uint64_t a0 = 0, a1 = 0;
  auto both = [&](uint64_t t) {
    a0 = gl::addc(gl::mulc(a0, beta0), t);
    a1 = gl::addc(gl::mulc(a1, beta1), t);
  };
  if constexpr (AIR == bpg::air::KECCAK_F) {
    *f = *v0 = *v1 = 0;
    if (pos < 23 || !gl::canon(row.loc(bpg::air::keccak::COL_G))) return;
  }
  *f = gl::canon(ctl::port_tuple<uint64_t>(bpg::air::Shape{AIR, 0, 0, 1}, col, row, both));
  if constexpr (AIR == bpg::air::KECCAK_F) {
    const CheckRow first{trace, nullptr, stride, 0, pos - 23, pos - 22, 0, nullptr};
#pragma unroll 1
    for (uint32_t j = ctl::TUPLE_LIMBS; j-- > 0;) both(first.loc(bpg::air::keccak::COL_A + j));
  }
  *v0 = a0;
  *v1 = a1;
}

// bit `pos % 64` of word `pos / 64` = bad; lane 0 of each wave (its row is a multiple of 64) writes the wave's word.
// Every lane of the wave must get here (no early return before it).
__device__ __forceinline__ void flag_rows(const CheckArgs& a, uint64_t pos, bool bad) {
  const unsigned long long b = __ballot(bad);
  if ((threadIdx.x & 63) == 0 && pos < ((uint64_t)1 << a.log_n)) {
    a.bitmap[pos >> 6] = b;
    if (b) atomicAdd(a.count, (unsigned long long)__popcll(b));
  }
}

}  // namespace chk
}  // namespace bpg
