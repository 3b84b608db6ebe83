// arithmetic_mod.hip -- the witness generator of the modular table (ADDMOD and MULMOD on 256-bit words, one operation per
// row), the second table proven by a constraint PROGRAM shipped with the Python package (proof_protocol_decoder_amd/
// arithmetic_mod.py, registered at run time).  include/bpg.h states the entries and the input words, AIRS.md section 2
// ("Modular (a shipped program)") the columns and why the constraints are sound.
//
// The column map below exists a second time, in the Python program; bp_arithmetic_mod_layout hands this one out so that
// arithmetic_mod.register() can refuse to run when the two differ.
#include "common.hpp"
#include "gl.hpp"
#include "word256.cuh"

namespace {

namespace md {
constexpr uint32_t LIMBS = 16, Q_LIMBS = 32, CARRY_BITS = 21, N_CARRIES = 31, CARRY_OFFSET = 1u << 20;
constexpr uint32_t COL_IS_ADDMOD = 0, COL_IS_MULMOD = 1, COL_G = 2, COL_Z = 3, COL_INV = 4;
constexpr uint32_t COL_A = 5, COL_B = COL_A + LIMBS, COL_M = COL_B + LIMBS, COL_RES = COL_M + LIMBS, COL_Q = COL_RES + LIMBS;
constexpr uint32_t COL_A_BITS = COL_Q + Q_LIMBS, COL_B_BITS = COL_A_BITS + 256, COL_M_BITS = COL_B_BITS + 256,
                   COL_Q_BITS = COL_M_BITS + 256, COL_R_BITS = COL_Q_BITS + 512, COL_D_BITS = COL_R_BITS + 256;
constexpr uint32_t COL_CARRY = COL_D_BITS + 256, COL_BORROW = COL_CARRY + N_CARRIES * CARRY_BITS, N_COLS = COL_BORROW + LIMBS;
constexpr uint32_t LAYOUT[] = {N_COLS, COL_IS_ADDMOD, COL_IS_MULMOD, COL_G, COL_Z, COL_INV, COL_A, COL_B, COL_M, COL_RES, COL_Q,
                               COL_A_BITS, COL_B_BITS, COL_M_BITS, COL_Q_BITS, COL_R_BITS, COL_D_BITS, COL_CARRY, CARRY_BITS,
                               CARRY_OFFSET, COL_BORROW};
constexpr uint32_t LAYOUT_WORDS = sizeof(LAYOUT) / sizeof(LAYOUT[0]);
static_assert(N_COLS == 2560, "AIRS.md section 2 lists 2560 columns");
}  // namespace md

using word256::limb;
using word256::Row;
using word256::sub256;
using word256::U256;

// A 512-bit word as eight named registers (two U256): the intermediate U and the quotient
struct U512 {
  U256 lo, hi;
};
template <uint32_t K>
__device__ __forceinline__ uint32_t limb(const U512& w) {
  if constexpr (K < 16) return limb<K>(w.lo);
  else return limb<K - 16>(w.hi);
}

// (*hi : returned) = x y + s + t, which is below 2^128
__device__ __forceinline__ uint64_t mul_add(uint64_t x, uint64_t y, uint64_t s, uint64_t t, uint64_t* hi) {
  uint64_t lo = x * y, h = __umul64hi(x, y);
  lo += s;
  h += lo < s;
  lo += t;
  h += lo < t;
  *hi = h;
  return lo;
}
// (t4 : t3 : t2 : t1 : t0) = (t3 : t2 : t1 : t0) + x w: one row of the 4 x 4 word product
__device__ __forceinline__ void mul_row(const U256& x, uint64_t w, uint64_t& t0, uint64_t& t1, uint64_t& t2, uint64_t& t3, uint64_t& t4) {
  uint64_t carry;
  t0 = mul_add(x.a, w, t0, 0, &carry);
  t1 = mul_add(x.b, w, t1, carry, &carry);
  t2 = mul_add(x.c, w, t2, carry, &carry);
  t3 = mul_add(x.d, w, t3, carry, &carry);
  t4 = carry;
}
__device__ __forceinline__ U512 mul256(const U256& x, const U256& y) {
  U512 u{{0, 0, 0, 0}, {0, 0, 0, 0}};
  mul_row(x, y.a, u.lo.a, u.lo.b, u.lo.c, u.lo.d, u.hi.a);
  mul_row(x, y.b, u.lo.b, u.lo.c, u.lo.d, u.hi.a, u.hi.b);
  mul_row(x, y.c, u.lo.c, u.lo.d, u.hi.a, u.hi.b, u.hi.c);
  mul_row(x, y.d, u.lo.d, u.hi.a, u.hi.b, u.hi.c, u.hi.d);
  return u;
}
__device__ __forceinline__ U512 add256(const U256& x, const U256& y) {
  U512 u{{0, 0, 0, 0}, {0, 0, 0, 0}};
  u.lo.a = x.a + y.a;
  uint64_t c = u.lo.a < x.a;
  uint64_t t = x.b + y.b;
  u.lo.b = t + c;
  c = (t < x.b) | (u.lo.b < t);
  t = x.c + y.c;
  u.lo.c = t + c;
  c = (t < x.c) | (u.lo.c < t);
  t = x.d + y.d;
  u.lo.d = t + c;
  u.hi.a = (t < x.d) | (u.lo.d < t);
  return u;
}

// sum_{i + j = K, i < 16, j < 16} a_i b_j, every limb number a compile-time number
template <uint32_t K, uint32_t I = (K < 16 ? 0 : K - 15)>
__device__ __forceinline__ uint64_t conv_left(const U256& a, const U256& b) {
  if constexpr (I > K || I > 15) return 0;
  else return (uint64_t)limb<I>(a) * limb<K - I>(b) + conv_left<K, I + 1>(a, b);
}
// sum_{i + j = K, i < 32, j <= 16} q_i M_j with M = m + z 2^256 (M_16 = z)
template <uint32_t K, uint32_t J = (K < 32 ? 0 : K - 31)>
__device__ __forceinline__ uint64_t conv_right(const U512& q, const U256& m, uint32_t z) {
  if constexpr (J > K || J > 16) return 0;
  else if constexpr (J == 16) return (uint64_t)limb<K - 16>(q) * z;
  else return (uint64_t)limb<K - J>(q) * limb<J>(m) + conv_right<K, J + 1>(q, m, z);
}

// What a row stores for product column K: limb K of q; for K < 16 limb K of a, b, m, r, d and the result and the carry
// bit of r + d + 1; and the SIGNED carry out of the column, L_K - R_K + c_(K-1) = 2^16 c_K, stored as c_K + 2^20 (columns
// 0 .. 30; the chain closes in column 31).  On an honest row the left side is a multiple of 2^16 and |c_K| < 2^20.
template <uint32_t K>
__device__ __forceinline__ void store_column(const Row& row, const U256& a, const U256& b, const U256& m, const U512& q, const U256& r,
                                             const U256& d, bool is_addmod, bool is_mulmod, bool m_zero, int64_t& carry, uint32_t& borrow) {
  const uint32_t qk = limb<K>(q);
  row.put(md::COL_Q + K, qk);
  row.put_bits(md::COL_Q_BITS + 16 * K, qk, 16);
  int64_t acc = carry + (int64_t)(is_mulmod ? conv_left<K>(a, b) : 0) - (int64_t)conv_right<K>(q, m, m_zero);
  if constexpr (K < md::LIMBS) {
    const uint32_t ak = limb<K>(a), bk = limb<K>(b), mk = limb<K>(m), rk = limb<K>(r), dk = limb<K>(d);
    row.put(md::COL_A + K, ak);
    row.put(md::COL_B + K, bk);
    row.put(md::COL_M + K, mk);
    row.put(md::COL_RES + K, m_zero ? 0u : rk);
    row.put_bits(md::COL_A_BITS + 16 * K, ak, 16);
    row.put_bits(md::COL_B_BITS + 16 * K, bk, 16);
    row.put_bits(md::COL_M_BITS + 16 * K, mk, 16);
    row.put_bits(md::COL_R_BITS + 16 * K, rk, 16);
    row.put_bits(md::COL_D_BITS + 16 * K, dk, 16);
    acc += (int64_t)(is_addmod ? ak + bk : 0u) - (int64_t)rk;
    // r_k + d_k + [K = 0] + carry bit in = m_k + 2^16 carry bit out; all zero when m = 0 (d = 0 there)
    borrow = m_zero ? 0u : (rk + dk + (K == 0 ? 1u : borrow)) >> 16;
    row.put(md::COL_BORROW + K, borrow);
  }
  carry = acc >> 16;  // arithmetic: the carries are signed
  if constexpr (K < md::N_CARRIES) row.put_bits(md::COL_CARRY + md::CARRY_BITS * K, (uint32_t)(carry + (int64_t)md::CARRY_OFFSET), md::CARRY_BITS);
}

template <uint32_t K>
__device__ __forceinline__ void store_columns(const Row& row, const U256& a, const U256& b, const U256& m, const U512& q, const U256& r,
                                              const U256& d, bool is_addmod, bool is_mulmod, bool m_zero, int64_t& carry, uint32_t& borrow) {
  if constexpr (K < md::Q_LIMBS) {
    store_column<K>(row, a, b, m, q, r, d, is_addmod, is_mulmod, m_zero, carry, borrow);
    store_columns<K + 1>(row, a, b, m, q, r, d, is_addmod, is_mulmod, m_zero, carry, borrow);
  }
}

template <uint32_t K = 0>
__device__ __forceinline__ uint32_t limb_sum(const U256& w) {
  if constexpr (K == md::LIMBS) return 0;
  else return limb<K>(w) + limb_sum<K + 1>(w);
}

// One operation per row, one lane per row.  inputs: [row][13] (include/bpg.h).  The lane forms U = a + b or a b in eight
// registers and divides by shift and subtract over (r : U) -- U gives a dividend bit to r at the top as it takes a
// quotient bit at the bottom, 512 steps --, then derives every column from q and r.  Stores are column-major.
__global__ void __launch_bounds__(256)
arithmetic_mod_trace_kernel(uint64_t* __restrict__ t, const uint64_t* __restrict__ inputs, uint32_t log_n) {
  const uint32_t n = 1u << log_n;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t* in = inputs + (uint64_t)i * 13;
  const uint64_t w0 = in[0];
  const uint32_t op = (uint32_t)w0 & 0xFFu;
  const bool is_addmod = op == 1, is_mulmod = op == 2, live = is_addmod | is_mulmod;
  // a padding row ignores its operand words and its exposed bit: U = 0, z = 1, the carry columns hold the offset
  const U256 zero{0, 0, 0, 0};
  const U256 a = live ? U256{in[1], in[2], in[3], in[4]} : zero;
  const U256 b = live ? U256{in[5], in[6], in[7], in[8]} : zero;
  const U256 m = live ? U256{in[9], in[10], in[11], in[12]} : zero;
  const bool m_zero = (m.a | m.b | m.c | m.d) == 0;

  U512 q = is_mulmod ? mul256(a, b) : add256(a, b);   // U now, the quotient after the loop
  U256 r = zero;
  if (m_zero) {  // M = 2^256: q = U >> 256, r = the low half of U
    r = q.lo;
    q.lo = q.hi;
    q.hi = zero;
  } else {
#pragma unroll 1
    for (uint32_t it = 0; it < 512; it++) {
      const uint32_t over = (uint32_t)(r.d >> 63);  // r < m before the shift, so 2 r + 1 may need a 257th bit
      r.d = (r.d << 1) | (r.c >> 63);
      r.c = (r.c << 1) | (r.b >> 63);
      r.b = (r.b << 1) | (r.a >> 63);
      r.a = (r.a << 1) | (q.hi.d >> 63);
      q.hi.d = (q.hi.d << 1) | (q.hi.c >> 63);
      q.hi.c = (q.hi.c << 1) | (q.hi.b >> 63);
      q.hi.b = (q.hi.b << 1) | (q.hi.a >> 63);
      q.hi.a = (q.hi.a << 1) | (q.lo.d >> 63);
      q.lo.d = (q.lo.d << 1) | (q.lo.c >> 63);
      q.lo.c = (q.lo.c << 1) | (q.lo.b >> 63);
      q.lo.b = (q.lo.b << 1) | (q.lo.a >> 63);
      q.lo.a <<= 1;
      uint32_t below;
      const U256 diff = sub256(r, m, &below);
      if (over | !below) {  // 2^256 over + r >= m: the difference is right modulo 2^256 and below m
        r = diff;
        q.lo.a |= 1;
      }
    }
  }
  uint32_t unused;
  // the slack of r < m: r + d + 1 = m
  const U256 d = m_zero ? zero : sub256(sub256(m, r, &unused), U256{1, 0, 0, 0}, &unused);

  const Row row{t + i, n};
  row.put(md::COL_IS_ADDMOD, is_addmod);
  row.put(md::COL_IS_MULMOD, is_mulmod);
  row.put(md::COL_G, live & (uint32_t)((w0 >> 8) & 1));
  row.put(md::COL_Z, m_zero);
  row.put(md::COL_INV, m_zero ? 0 : gl::inv((uint64_t)limb_sum(m)));
  int64_t carry = 0;
  uint32_t borrow = 0;
  store_columns<0>(row, a, b, m, q, r, d, is_addmod, is_mulmod, m_zero, carry, borrow);
}

}  // namespace

extern "C" {

int bp_arithmetic_mod_layout(uint32_t* out, size_t n_words) {
  if (!out || n_words < md::LAYOUT_WORDS)
    return bpg::fail(BP_ERR_INVALID_INPUT, "bp_arithmetic_mod_layout: the layout is %u words", md::LAYOUT_WORDS);
  for (uint32_t k = 0; k < md::LAYOUT_WORDS; k++) out[k] = md::LAYOUT[k];
  return BP_OK;
}

int bp_arithmetic_mod_trace(const uint64_t* d_inputs, uint32_t log_n, uint64_t* d_trace_out, void* stream) try {
  if (!d_inputs) return bpg::fail(BP_ERR_INVALID_INPUT, "bp_arithmetic_mod_trace: null inputs (this table has no seeded draw)");
  if (!d_trace_out) return bpg::fail(BP_ERR_INVALID_INPUT, "bp_arithmetic_mod_trace: null output");
  if (log_n < 4 || log_n > 26) return bpg::fail(BP_ERR_INVALID_INPUT, "bp_arithmetic_mod_trace: log_n out of range");
  arithmetic_mod_trace_kernel<<<bpg::ceil_div((uint64_t)1 << log_n, 256), 256, 0, bpg::as_stream(stream)>>>(d_trace_out, d_inputs, log_n);
  BPG_LAUNCH_CHECK();
  return BP_OK;
}
BPG_ABI_CATCH("bp_arithmetic_mod_trace")

}  // extern "C"
