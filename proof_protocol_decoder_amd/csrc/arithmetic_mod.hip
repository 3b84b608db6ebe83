// arithmetic_mod.hip -- the witness generator of the modular table (ADDMOD and MULMOD on 256-bit words, one operation per
// row), the second table proven by a constraint PROGRAM shipped with the Python package (proof_protocol_decoder_amd/
// arithmetic_mod.py, registered at run time).  include/bpg.h states the entries and the input words, AIRS.md section 2
// ("Modular (a shipped program)") the columns and why the constraints are sound.
//
// The column map below exists a second time, in the Python program; bp_arithmetic_mod_layout hands this one out so that
// arithmetic_mod.register() can refuse to run when the two differ.  What this table has in common with the division
// table is in word256.cuh: this file keeps the map, U = a + b or a b in 512 bits, the signed product columns and the kernel.
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
constexpr word256::SharedCols SHARED = {COL_IS_ADDMOD, COL_IS_MULMOD, COL_G, COL_Z, COL_INV, COL_R_BITS, COL_D_BITS, COL_BORROW};
static_assert(N_COLS == 2560, "AIRS.md section 2 lists 2560 columns");
}  // namespace md

using word256::limb;
using word256::Row;
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
  int64_t acc = carry + (int64_t)(is_mulmod ? word256::conv<K>(a, b) : 0) - (int64_t)conv_right<K>(q, m, m_zero);
  if constexpr (K < md::LIMBS) {
    const uint32_t ak = limb<K>(a), bk = limb<K>(b), mk = limb<K>(m), rk = limb<K>(r);
    row.put(md::COL_A + K, ak);
    row.put(md::COL_B + K, bk);
    row.put(md::COL_M + K, mk);
    row.put(md::COL_RES + K, m_zero ? 0u : rk);
    row.put_bits(md::COL_A_BITS + 16 * K, ak, 16);
    row.put_bits(md::COL_B_BITS + 16 * K, bk, 16);
    row.put_bits(md::COL_M_BITS + 16 * K, mk, 16);
    row.template put_remainder_limb<K>(md::SHARED, r, d, m_zero, borrow);
    acc += (int64_t)(is_addmod ? ak + bk : 0u) - (int64_t)rk;
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

// One operation per row, one lane per row.  inputs: [row][13] (include/bpg.h).  The lane forms U = a + b or a b in eight
// registers and divides by shift and subtract over (r : U) -- U gives a dividend bit to r at the top as it takes a
// quotient bit at the bottom, 512 steps --, then derives every column from q and r.  Stores are column-major.
__global__ void __launch_bounds__(256)
arithmetic_mod_trace_kernel(uint64_t* __restrict__ t, const uint64_t* __restrict__ inputs, uint32_t log_n) {
  const uint32_t n = 1u << log_n;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t* in = inputs + (uint64_t)i * 13;
  const word256::Head h(in[0]);
  const bool is_addmod = h.op_a, is_mulmod = h.op_b;
  // a padding row ignores its operand words and its exposed bit: U = 0, z = 1, the carry columns hold the offset
  const U256 zero{0, 0, 0, 0};
  const U256 a = word256::operand<0>(in, h.live), b = word256::operand<1>(in, h.live), m = word256::operand<2>(in, h.live);
  const bool m_zero = word256::is_zero(m);

  U512 q = is_mulmod ? mul256(a, b) : add256(a, b);   // U now, the quotient after the loop
  U256 r = zero;
  if (m_zero) {  // M = 2^256: q = U >> 256, r = the low half of U
    r = q.lo;
    q.lo = q.hi;
    q.hi = zero;
  } else {
#pragma unroll 1
    for (uint32_t it = 0; it < 512; it++) {
      const uint64_t bit = word256::shift_in(q.hi, word256::shift_in(q.lo, 0));
      word256::subtract_step(r, m, bit, q.lo.a);
    }
  }
  const U256 d = word256::slack(m, r, m_zero);

  const Row row{t + i, n};
  row.put_head(md::SHARED, h, m, m_zero);
  int64_t carry = 0;
  uint32_t borrow = 0;
  store_columns<0>(row, a, b, m, q, r, d, is_addmod, is_mulmod, m_zero, carry, borrow);
}

}  // namespace

extern "C" {

int bp_arithmetic_mod_layout(uint32_t* out, size_t n_words) { return word256::layout_entry("bp_arithmetic_mod_layout", md::LAYOUT, out, n_words); }

int bp_arithmetic_mod_trace(const uint64_t* d_inputs, uint32_t log_n, uint64_t* d_trace_out, void* stream) try {
  return word256::trace_entry("bp_arithmetic_mod_trace", arithmetic_mod_trace_kernel, d_inputs, log_n, d_trace_out, stream);
}
BPG_ABI_CATCH("bp_arithmetic_mod_trace")

}  // extern "C"
