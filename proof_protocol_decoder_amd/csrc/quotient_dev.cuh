// quotient_dev.cuh -- the device pieces every K5 quotient kernel is made of (stark_kernels.hip: the built-in AIRs;
// air_program.hip: registered programs): a point of the LDE coset as air.hpp's row accessors read it, and the constraint
// consumer that folds (index, value) pairs with the alpha-power table.  One definition, so the fold of every kernel --
// and with it every quotient value -- is the same bit for bit.
#pragma once
#include "gl.hpp"
#include "stark_kernels.hpp"

namespace bpg {
namespace k5 {

// w_n^m from the half-size table tw[e] = w_n^e, e < n/2
__device__ __forceinline__ uint64_t root_pow(const uint64_t* __restrict__ tw, uint32_t log_n, uint32_t m) {
  if (log_n == 0) return 1;
  const uint32_t half = 1u << (log_n - 1);
  uint64_t w = tw[m & (half - 1)];
  return (m & half) ? gl::negc(w) : w;
}
struct RowPoint {
  uint64_t z_last, l_first, l_last, x;
};
__device__ __forceinline__ RowPoint row_point(const bpg::QuotArgs& q, uint32_t t, uint32_t m) {
  // per-coset constants from the table alpha_table_kernel left behind the alpha powers (t is a per-lane value:
  // indexing the kernel-argument arrays with it would pull all 48 words into SGPRs)
  const uint64_t* coset = q.apow + 2 * (size_t)q.n_constraints;
  const uint64_t x = gl::mulc(coset[t], root_pow(q.tw_n, q.log_n, m));
  const uint64_t zh = coset[16 + t];
  RowPoint p;
  p.x = x;
  p.z_last = gl::subc(x, q.g_inv);
  const uint64_t zn = gl::mulc(zh, q.n_inv);
  // both Lagrange denominators with one inversion (x is off the subgroup: neither is zero)
  const uint64_t df = gl::subc(x, 1), dl = gl::subc(gl::mulc(q.g, x), 1);
  const uint64_t both = gl::mulc(zn, gl::inv(gl::mulc(df, dl)));
  p.l_first = gl::mulc(both, dl);
  p.l_last = gl::mulc(both, df);
  return p;
}
struct DevRow {  // one point of the coset: column-major matrices, lanes = consecutive rows (coalesced)
  const uint64_t *trace, *aux_, *cst_;
  uint64_t ts, as, cs, pos, pos_next;
  uint64_t xv;          // the point itself
  const uint64_t* pub_;  // the table's public inputs (kernel arguments)
  __device__ __forceinline__ uint64_t x() const { return xv; }
  __device__ __forceinline__ uint64_t pub(uint32_t j) const { return pub_[j]; }
  __device__ __forceinline__ uint64_t loc(uint32_t c) const { return trace[(uint64_t)c * ts + pos]; }
  __device__ __forceinline__ uint64_t nxt(uint32_t c) const { return trace[(uint64_t)c * ts + pos_next]; }
  __device__ __forceinline__ uint64_t cst(uint32_t k) const { return cst_[(uint64_t)k * cs + pos]; }
  __device__ __forceinline__ uint64_t aux(uint32_t k) const { return aux_[(uint64_t)k * as + pos]; }
  __device__ __forceinline__ uint64_t aux_nxt(uint32_t k) const { return aux_[(uint64_t)k * as + pos_next]; }
};
struct DevEmit {  // the constraint consumer: two constraints (x two challenges) per dot_mad4
  const uint64_t* apow;  // [2][T]: alpha_j^e (wave-uniform reads)
  uint32_t T;
  RowPoint rp;
  gl::DotAcc acc[4];  // 0, 1: challenge 0 / 1 of the first constraint of a pair; 2, 3: of the second
  uint64_t pend_v;
  uint32_t pend_e;
  bool has;
  __device__ __forceinline__ void push(uint32_t idx, uint64_t v) {
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
  __device__ __forceinline__ void transition(uint32_t idx, uint64_t v) { push(idx, gl::mulc(v, rp.z_last)); }
  __device__ __forceinline__ void first(uint32_t idx, uint64_t v) { push(idx, gl::mulc(v, rp.l_first)); }
  __device__ __forceinline__ void last(uint32_t idx, uint64_t v) { push(idx, gl::mulc(v, rp.l_last)); }
  // the same four by a run-time (wave-uniform) kind, through one push: the program interpreter's (air_program.hpp)
  __device__ __forceinline__ void emit(uint32_t kind, uint32_t idx, uint64_t v) {
    if (kind) v = gl::mulc(v, kind == 1 ? rp.z_last : kind == 2 ? rp.l_first : rp.l_last);
    push(idx, v);
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

}  // namespace k5
}  // namespace bpg
