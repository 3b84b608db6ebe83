// word256.cuh -- what the witness kernels of the five shipped tables (arithmetic_div.hip, arithmetic_mod.hip,
// arithmetic_shift.hip, arithmetic_sdiv.hip, arithmetic_exp.hip) share: a 256-bit word in named registers, its 16-bit limbs
// by compile-time number, a column of the limb product (conv), the shift-and-subtract step and the whole 256-bit division
// made of it (divide), a lane's view of its trace row with the stores every quotient / remainder / slack table makes, and
// the host side of the two C entries a table has.  A table's .hip file keeps its column map, its store_limb(s) and its
// kernel.  The shift table, which has no quotient, uses U256, limb, Head3, operand, Row::put / put_bits and the two
// entries; the division and the signed table divide by divide, the signed one between negate / magnitude; the modular
// table has a 512-bit loop of its own over shift_in / subtract_step; the exponentiation table, whose rows are steps of a
// chain, uses U256, limb, conv, mul_low, Row::put / put_bits and layout_entry.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "common.hpp"
#include "gl.hpp"

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
// -w modulo 2^256, and |W| of the two's-complement word w = W mod 2^256 (2^255 for the most negative one)
__device__ __forceinline__ U256 negate(const U256& w) {
  uint32_t unused;
  return sub256(U256{0, 0, 0, 0}, w, &unused);
}
__device__ __forceinline__ U256 magnitude(const U256& w) { return (w.d >> 63) ? negate(w) : w; }
// x y modulo 2^256: the schoolbook product over 64-bit words, columns 0 .. 3 only.  `carry` counts the wraps of a column's
// sum, which belong to the next column; the last column wraps freely.
__device__ __forceinline__ void add_wrapping(uint64_t& acc, uint64_t& carry, uint64_t v) {
  acc += v;
  carry += acc < v;
}
__device__ __forceinline__ U256 mul_low(const U256& x, const U256& y) {
  U256 r;
  r.a = x.a * y.a;
  uint64_t acc = __umul64hi(x.a, y.a), carry = 0;
  add_wrapping(acc, carry, x.a * y.b);
  add_wrapping(acc, carry, x.b * y.a);
  r.b = acc;
  acc = carry;
  carry = 0;
  add_wrapping(acc, carry, __umul64hi(x.a, y.b));
  add_wrapping(acc, carry, __umul64hi(x.b, y.a));
  add_wrapping(acc, carry, x.a * y.c);
  add_wrapping(acc, carry, x.b * y.b);
  add_wrapping(acc, carry, x.c * y.a);
  r.c = acc;
  r.d = carry + __umul64hi(x.a, y.c) + __umul64hi(x.b, y.b) + __umul64hi(x.c, y.a) + x.a * y.d + x.b * y.c + x.c * y.b + x.d * y.a;
  return r;
}
// limb K (16 bits) of a word, K a compile-time number
template <uint32_t K>
__device__ __forceinline__ uint32_t limb(const U256& w) {
  const uint64_t v = K < 4 ? w.a : K < 8 ? w.b : K < 12 ? w.c : w.d;
  return (uint32_t)(v >> (16 * (K & 3))) & 0xFFFFu;
}
template <uint32_t K = 0>
__device__ __forceinline__ uint32_t limb_sum(const U256& w) {
  if constexpr (K == 16) return 0;
  else return limb<K>(w) + limb_sum<K + 1>(w);
}
// sum_{i + j = K, i < 16, j < 16} x_i y_j, column K of the limb product: K and every limb number a compile-time number,
// at most sixteen terms, so below 16 (2^16 - 1)^2
template <uint32_t K, uint32_t I = (K < 16 ? 0 : K - 15)>
__device__ __forceinline__ uint64_t conv(const U256& x, const U256& y) {
  if constexpr (I > K || I > 15) return 0;
  else return (uint64_t)limb<I>(x) * limb<K - I>(y) + conv<K, I + 1>(x, y);
}

// ---- division by shift and subtract
// w = 2 w + in; returns the bit that leaves at the top.  A dividend of 512 bits is two of these, the low half's bit out
// the high half's bit in.
__device__ __forceinline__ uint64_t shift_in(U256& w, uint64_t in) {
  const uint64_t out = w.d >> 63;
  w.d = (w.d << 1) | (w.c >> 63);
  w.c = (w.c << 1) | (w.b >> 63);
  w.b = (w.b << 1) | (w.a >> 63);
  w.a = (w.a << 1) | in;
  return out;
}
// One step on the remainder: r = 2 r + the next dividend bit, less the divisor if that fits -- the quotient bit, set at
// the bottom of `quotient_low`, the dividend's lowest register, which has just been shifted.
__device__ __forceinline__ void subtract_step(U256& r, const U256& divisor, uint64_t dividend_bit, uint64_t& quotient_low) {
  const uint32_t over = (uint32_t)shift_in(r, dividend_bit);  // r < divisor before the shift, so 2 r + 1 may need a 257th bit
  uint32_t below;
  const U256 diff = sub256(r, divisor, &below);
  if (over | !below) {  // 2^256 over + r >= divisor: the difference is right modulo 2^256 and below the divisor
    r = diff;
    quotient_low |= 1;
  }
}
// the slack d of r < y: r + d + 1 = y; zero when y = 0
__device__ __forceinline__ U256 slack(const U256& y, const U256& r, bool y_zero) {
  uint32_t unused;
  return y_zero ? U256{0, 0, 0, 0} : sub256(sub256(y, r, &unused), U256{1, 0, 0, 0}, &unused);
}
// q, r and the slack d of dividend = q divisor + r, r + d + 1 = divisor, over the register pair (r : q): q starts as the
// dividend and gives a dividend bit to r at the top as it takes a quotient bit at the bottom.  The EVM's x / 0 is q = 0,
// r = x, d = 0; the caller has tested the divisor already and says so in `divisor_zero`.
struct Division {
  U256 q, r, d;
};
__device__ __forceinline__ Division divide(const U256& dividend, const U256& divisor, bool divisor_zero) {
  Division v{dividend, U256{0, 0, 0, 0}, U256{0, 0, 0, 0}};
#pragma unroll 1
  for (uint32_t it = 0; it < 256; it++) {
    const uint64_t bit = shift_in(v.q, 0);
    subtract_step(v.r, divisor, bit, v.q.a);
  }
  if (divisor_zero) {  // the loop subtracted zero 256 times: q is all ones, r is the dividend
    v.q = U256{0, 0, 0, 0};
    v.r = dividend;
  }
  v.d = slack(divisor, v.r, divisor_zero);
  return v;
}

// ---- a row's inputs: word 0 = op byte | exposed << 8, then four words per operand (include/bpg.h)
struct Head {
  uint64_t w0;
  bool op_a, op_b, live;  // op 1, op 2, either: anything else is a padding row
  __device__ __forceinline__ explicit Head(uint64_t word0)
      : w0(word0), op_a(((uint32_t)word0 & 0xFFu) == 1), op_b(((uint32_t)word0 & 0xFFu) == 2), live(op_a | op_b) {}
  __device__ __forceinline__ uint32_t g() const { return live & (uint32_t)((w0 >> 8) & 1); }  // exposed, on a live row only
};
// the same for a table of three operations (op bytes 1, 2, 3)
struct Head3 {
  uint64_t w0;
  bool op_a, op_b, op_c, live;
  __device__ __forceinline__ explicit Head3(uint64_t word0)
      : w0(word0), op_a(((uint32_t)word0 & 0xFFu) == 1), op_b(((uint32_t)word0 & 0xFFu) == 2), op_c(((uint32_t)word0 & 0xFFu) == 3),
        live(op_a | op_b | op_c) {}
  __device__ __forceinline__ uint32_t g() const { return live & (uint32_t)((w0 >> 8) & 1); }
};
// operand J of the row at `in`; a padding row ignores its operand words: they read as zero
template <uint32_t J>
__device__ __forceinline__ U256 operand(const uint64_t* in, bool live) {
  return live ? U256{in[1 + 4 * J], in[2 + 4 * J], in[3 + 4 * J], in[4 + 4 * J]} : U256{0, 0, 0, 0};
}
__device__ __forceinline__ bool is_zero(const U256& w) { return (w.a | w.b | w.c | w.d) == 0; }

// the columns every such table has, by the table's own numbers: the two flags, g, z, inv; the bits of r and of the
// slack; the carry bits of r + d + 1
struct SharedCols {
  uint32_t op_a, op_b, g, z, inv, r_bits, d_bits, borrow;
};

struct Row {
  uint64_t* t;  // the trace at this lane's row: column c at t[c * n]
  uint64_t n;
  __device__ __forceinline__ void put(uint32_t col, uint64_t v) const { t[(uint64_t)col * n] = v; }
  // `count` bit columns from `col`: bit j of v at col + j
  __device__ __forceinline__ void put_bits(uint32_t col, uint32_t v, uint32_t count) const {
#pragma unroll 1
    for (uint32_t j = 0; j < count; j++) put(col + j, (v >> j) & 1u);
  }
  // the flags, the filter, z = [y = 0] and the inverse of the sum of y's limbs (zero with z)
  __device__ __forceinline__ void put_head(const SharedCols& c, const Head& h, const U256& y, bool y_zero) const {
    put(c.op_a, h.op_a);
    put(c.op_b, h.op_b);
    put(c.g, h.g());
    put(c.z, y_zero);
    put(c.inv, y_zero ? 0 : gl::inv((uint64_t)limb_sum(y)));
  }
  // limb K of r and of d, and the chain r_k + d_k + [K = 0] + carry bit in = y_k + 2^16 carry bit out; all zero when
  // y = 0 (d = 0 there, the bits too)
  template <uint32_t K>
  __device__ __forceinline__ void put_remainder_limb(const SharedCols& c, const U256& r, const U256& d, bool y_zero, uint32_t& borrow) const {
    const uint32_t rk = limb<K>(r), dk = limb<K>(d);
    put_bits(c.r_bits + 16 * K, rk, 16);
    put_bits(c.d_bits + 16 * K, dk, 16);
    borrow = y_zero ? 0u : (rk + dk + (K == 0 ? 1u : borrow)) >> 16;
    put(c.borrow + K, borrow);
  }
};

// ---- the host side of a table's two C entries; `name` is the entry's, for the error text
template <size_t N>
inline int layout_entry(const char* name, const uint32_t (&layout)[N], uint32_t* out, size_t n_words) {
  if (!out || n_words < N) return bpg::fail(BP_ERR_INVALID_INPUT, "%s: the layout is %u words", name, (uint32_t)N);
  for (size_t k = 0; k < N; k++) out[k] = layout[k];
  return BP_OK;
}
using TraceKernel = void (*)(uint64_t* t, const uint64_t* inputs, uint32_t log_n);  // one lane per row, 256 a workgroup
inline int trace_entry(const char* name, TraceKernel kernel, const uint64_t* d_inputs, uint32_t log_n, uint64_t* d_trace_out, void* stream) {
  if (!d_inputs) return bpg::fail(BP_ERR_INVALID_INPUT, "%s: null inputs (this table has no seeded draw)", name);
  if (!d_trace_out) return bpg::fail(BP_ERR_INVALID_INPUT, "%s: null output", name);
  if (log_n < 4 || log_n > 26) return bpg::fail(BP_ERR_INVALID_INPUT, "%s: log_n out of range", name);
  kernel<<<bpg::ceil_div((uint64_t)1 << log_n, 256), 256, 0, bpg::as_stream(stream)>>>(d_trace_out, d_inputs, log_n);
  BPG_LAUNCH_CHECK();
  return BP_OK;
}

}  // namespace word256
