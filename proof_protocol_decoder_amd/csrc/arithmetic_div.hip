// arithmetic_div.hip -- the witness generator of the division table (DIV and MOD on 256-bit words, one operation per
// row), a table proven by a constraint PROGRAM shipped with the Python package (proof_protocol_decoder_amd/
// arithmetic_div.py, registered at run time) instead of a built-in AIR.  include/bpg.h states the entries and the input
// words, AIRS.md section 2 ("Division (a shipped program)") the columns and why the constraints are sound.
//
// The column map below exists a second time, in the Python program; bp_arithmetic_div_layout hands this one out so that
// arithmetic_div.register() can refuse to run when the two differ.  Everything a quotient / remainder / slack table
// over 16-bit limbs has in common with the next one is in word256.cuh: this file keeps the map, q y + r = x and the kernel.
#include "word256.cuh"

namespace {

namespace dv {
constexpr uint32_t LIMBS = 16, CARRY_BITS = 19, N_CARRIES = 15;
constexpr uint32_t COL_IS_DIV = 0, COL_IS_MOD = 1, COL_G = 2, COL_Z = 3, COL_INV = 4;
constexpr uint32_t COL_X = 5, COL_Y = COL_X + LIMBS, COL_RES = COL_Y + LIMBS, COL_Q = COL_RES + LIMBS;
constexpr uint32_t COL_X_BITS = COL_Q + LIMBS, COL_Y_BITS = COL_X_BITS + 256, COL_Q_BITS = COL_Y_BITS + 256,
                   COL_R_BITS = COL_Q_BITS + 256, COL_D_BITS = COL_R_BITS + 256;
constexpr uint32_t COL_CARRY = COL_D_BITS + 256, COL_BORROW = COL_CARRY + N_CARRIES * CARRY_BITS, N_COLS = COL_BORROW + LIMBS;
constexpr uint32_t LAYOUT[] = {N_COLS, COL_IS_DIV, COL_IS_MOD, COL_G, COL_Z, COL_INV, COL_X, COL_Y, COL_RES, COL_Q, COL_X_BITS,
                               COL_Y_BITS, COL_Q_BITS, COL_R_BITS, COL_D_BITS, COL_CARRY, CARRY_BITS, COL_BORROW};
constexpr word256::SharedCols SHARED = {COL_IS_DIV, COL_IS_MOD, COL_G, COL_Z, COL_INV, COL_R_BITS, COL_D_BITS, COL_BORROW};
}  // namespace dv

using word256::limb;
using word256::Row;
using word256::U256;

// what a row stores for limb K of x, y, q, r, d and the result, and the product column K: the carry out of it (columns
// 0 .. 14; the honest carry out of column 15 is zero because q y + r = x < 2^256) and the carry bit of r + d + 1
template <uint32_t K>
__device__ __forceinline__ void store_limb(const Row& row, const U256& x, const U256& y, const U256& q, const U256& r, const U256& d,
                                           const U256& res, uint64_t conv, uint64_t& carry, uint32_t& borrow, bool y_zero) {
  const uint32_t xk = limb<K>(x), yk = limb<K>(y), qk = limb<K>(q);
  row.put(dv::COL_X + K, xk);
  row.put(dv::COL_Y + K, yk);
  row.put(dv::COL_Q + K, qk);
  row.put(dv::COL_RES + K, limb<K>(res));
  row.put_bits(dv::COL_X_BITS + 16 * K, xk, 16);
  row.put_bits(dv::COL_Y_BITS + 16 * K, yk, 16);
  row.put_bits(dv::COL_Q_BITS + 16 * K, qk, 16);
  // conv + r_k + carry in = x_k + 2^16 carry out: below 16 * 2^32 + 2^16 + 2^19, and at least x_k on an honest row
  carry = (conv + limb<K>(r) + carry - xk) >> 16;
  if constexpr (K < dv::N_CARRIES) row.put_bits(dv::COL_CARRY + dv::CARRY_BITS * K, (uint32_t)carry, dv::CARRY_BITS);
  row.template put_remainder_limb<K>(dv::SHARED, r, d, y_zero, borrow);
}

template <uint32_t K>
__device__ __forceinline__ void store_limbs(const Row& row, const U256& x, const U256& y, const U256& q, const U256& r, const U256& d,
                                            const U256& res, uint64_t& carry, uint32_t& borrow, bool y_zero) {
  if constexpr (K < dv::LIMBS) {
    store_limb<K>(row, x, y, q, r, d, res, word256::conv<K>(q, y), carry, borrow, y_zero);
    store_limbs<K + 1>(row, x, y, q, r, d, res, carry, borrow, y_zero);
  }
}

// One operation per row, one lane per row.  inputs: [row][9] (include/bpg.h).  The lane divides by shift and subtract
// (word256::divide), then derives every column from q and r.  Stores are column-major, so a wave's are contiguous.
__global__ void __launch_bounds__(256)
arithmetic_div_trace_kernel(uint64_t* __restrict__ t, const uint64_t* __restrict__ inputs, uint32_t log_n) {
  const uint32_t n = 1u << log_n;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t* in = inputs + (uint64_t)i * 9;
  const word256::Head h(in[0]);
  // a padding row ignores its operand words and its exposed bit: it is the all-zero row with z = 1
  const U256 zero{0, 0, 0, 0};
  const U256 x = word256::operand<0>(in, h.live), y = word256::operand<1>(in, h.live);
  const bool y_zero = word256::is_zero(y);
  const auto [q, r, d] = word256::divide(x, y, y_zero);
  const U256 res = y_zero ? zero : h.op_a ? q : r;  // (a padding row has y = 0)

  const Row row{t + i, n};
  row.put_head(dv::SHARED, h, y, y_zero);
  uint64_t carry = 0;
  uint32_t borrow = 0;
  store_limbs<0>(row, x, y, q, r, d, res, carry, borrow, y_zero);
}

}  // namespace

extern "C" {

int bp_arithmetic_div_layout(uint32_t* out, size_t n_words) { return word256::layout_entry("bp_arithmetic_div_layout", dv::LAYOUT, out, n_words); }

int bp_arithmetic_div_trace(const uint64_t* d_inputs, uint32_t log_n, uint64_t* d_trace_out, void* stream) try {
  return word256::trace_entry("bp_arithmetic_div_trace", arithmetic_div_trace_kernel, d_inputs, log_n, d_trace_out, stream);
}
BPG_ABI_CATCH("bp_arithmetic_div_trace")

}  // extern "C"
