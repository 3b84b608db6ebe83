// arithmetic_sdiv.hip -- the witness generator of the signed table (SDIV and SMOD on 256-bit words, one operation per
// row), the fourth table proven by a constraint PROGRAM shipped with the Python package (proof_protocol_decoder_amd/
// arithmetic_sdiv.py, registered at run time) instead of a built-in AIR.  include/bpg.h states the entries and the input
// words, AIRS.md section 2 ("Signed (a shipped program)") the columns and why the constraints are sound.
//
// The column map below exists a second time, in the Python program; bp_arithmetic_sdiv_layout hands this one out so that
// arithmetic_sdiv.register() can refuse to run when the two differ.  The table is the division table's core on the
// magnitudes ax = |X|, ay = |Y| between three conditional negations (x -> ax, y -> ay, m -> res); what it shares with
// the other tables is in word256.cuh: this file keeps the map, the chains' carry bits, q ay + r = ax and the kernel.
#include "word256.cuh"

namespace {

namespace sd {
constexpr uint32_t LIMBS = 16, CARRY_BITS = 19, N_CARRIES = 15;
constexpr uint32_t COL_IS_SDIV = 0, COL_IS_SMOD = 1, COL_G = 2, COL_Z = 3, COL_INV = 4, COL_NEG = 5;
constexpr uint32_t COL_X = 6, COL_Y = COL_X + LIMBS, COL_RES = COL_Y + LIMBS, COL_Q = COL_RES + LIMBS, COL_AY = COL_Q + LIMBS,
                   COL_M = COL_AY + LIMBS;
constexpr uint32_t COL_X_BITS = COL_M + LIMBS, COL_Y_BITS = COL_X_BITS + 256, COL_RES_BITS = COL_Y_BITS + 256,
                   COL_AX_BITS = COL_RES_BITS + 256, COL_AY_BITS = COL_AX_BITS + 256, COL_Q_BITS = COL_AY_BITS + 256,
                   COL_R_BITS = COL_Q_BITS + 256, COL_D_BITS = COL_R_BITS + 256;
constexpr uint32_t COL_CARRY = COL_D_BITS + 256, COL_BORROW = COL_CARRY + N_CARRIES * CARRY_BITS, COL_X_CHAIN = COL_BORROW + LIMBS,
                   COL_Y_CHAIN = COL_X_CHAIN + LIMBS, COL_RES_CHAIN = COL_Y_CHAIN + LIMBS, N_COLS = COL_RES_CHAIN + LIMBS;
constexpr uint32_t LAYOUT[] = {N_COLS, COL_IS_SDIV, COL_IS_SMOD, COL_G, COL_Z, COL_INV, COL_NEG, COL_X, COL_Y, COL_RES, COL_Q, COL_AY,
                               COL_M, COL_X_BITS, COL_Y_BITS, COL_RES_BITS, COL_AX_BITS, COL_AY_BITS, COL_Q_BITS, COL_R_BITS,
                               COL_D_BITS, COL_CARRY, CARRY_BITS, COL_BORROW, COL_X_CHAIN, COL_Y_CHAIN, COL_RES_CHAIN};
constexpr word256::SharedCols SHARED = {COL_IS_SDIV, COL_IS_SMOD, COL_G, COL_Z, COL_INV, COL_R_BITS, COL_D_BITS, COL_BORROW};
}  // namespace sd

using word256::limb;
using word256::Row;
using word256::U256;

// the carry bits of the three chains v + w = 2^256 c_15 (x + ax, y + ay, m + res), each zero where its sign is
struct Chains {
  uint32_t x, y, res;
};

// limb K of a conditional negation: the carry bit out of v_k + w_k + carry in, zero where the word is not negated
template <uint32_t K>
__device__ __forceinline__ void put_chain_limb(const Row& row, uint32_t col, bool sign, const U256& v, const U256& w, uint32_t& carry) {
  carry = sign ? (limb<K>(v) + limb<K>(w) + carry) >> 16 : 0u;
  row.put(col + K, carry);
}

// what a row stores for limb K of x, y, res, q, ay, m, ax, r, d, and the product column K: the carry out of it (columns
// 0 .. 14; the honest carry out of column 15 is zero because q ay + r = ax < 2^256) and the carry bits of r + d + 1 and of
// the three negations
template <uint32_t K>
__device__ __forceinline__ void store_limb(const Row& row, const U256& x, const U256& y, const U256& ax, const U256& ay, const U256& q,
                                           const U256& r, const U256& d, const U256& m, const U256& res, uint64_t conv, uint64_t& carry,
                                           uint32_t& borrow, Chains& chains, bool sx, bool sy, bool neg, bool y_zero) {
  const uint32_t xk = limb<K>(x), yk = limb<K>(y), resk = limb<K>(res), qk = limb<K>(q), axk = limb<K>(ax), ayk = limb<K>(ay);
  row.put(sd::COL_X + K, xk);
  row.put(sd::COL_Y + K, yk);
  row.put(sd::COL_RES + K, resk);
  row.put(sd::COL_Q + K, qk);
  row.put(sd::COL_AY + K, ayk);
  row.put(sd::COL_M + K, limb<K>(m));
  row.put_bits(sd::COL_X_BITS + 16 * K, xk, 16);
  row.put_bits(sd::COL_Y_BITS + 16 * K, yk, 16);
  row.put_bits(sd::COL_RES_BITS + 16 * K, resk, 16);
  row.put_bits(sd::COL_AX_BITS + 16 * K, axk, 16);
  row.put_bits(sd::COL_AY_BITS + 16 * K, ayk, 16);
  row.put_bits(sd::COL_Q_BITS + 16 * K, qk, 16);
  // conv + r_k + carry in = ax_k + 2^16 carry out: below 16 * 2^32 + 2^16 + 2^19, and at least ax_k on an honest row
  carry = (conv + limb<K>(r) + carry - axk) >> 16;
  if constexpr (K < sd::N_CARRIES) row.put_bits(sd::COL_CARRY + sd::CARRY_BITS * K, (uint32_t)carry, sd::CARRY_BITS);
  row.template put_remainder_limb<K>(sd::SHARED, r, d, y_zero, borrow);
  put_chain_limb<K>(row, sd::COL_X_CHAIN, sx, x, ax, chains.x);
  put_chain_limb<K>(row, sd::COL_Y_CHAIN, sy, y, ay, chains.y);
  put_chain_limb<K>(row, sd::COL_RES_CHAIN, neg, m, res, chains.res);
}

template <uint32_t K>
__device__ __forceinline__ void store_limbs(const Row& row, const U256& x, const U256& y, const U256& ax, const U256& ay, const U256& q,
                                            const U256& r, const U256& d, const U256& m, const U256& res, uint64_t& carry,
                                            uint32_t& borrow, Chains& chains, bool sx, bool sy, bool neg, bool y_zero) {
  if constexpr (K < sd::LIMBS) {
    store_limb<K>(row, x, y, ax, ay, q, r, d, m, res, word256::conv<K>(q, ay), carry, borrow, chains, sx, sy, neg, y_zero);
    store_limbs<K + 1>(row, x, y, ax, ay, q, r, d, m, res, carry, borrow, chains, sx, sy, neg, y_zero);
  }
}

// One operation per row, one lane per row.  inputs: [row][9] (include/bpg.h).  The lane takes the magnitudes of x and y,
// divides them by shift and subtract (word256::divide, as the division kernel does), picks the magnitude m of the result,
// negates it under the result's sign, then derives every column.  Stores are column-major, so a wave's are contiguous.
__global__ void __launch_bounds__(256)
arithmetic_sdiv_trace_kernel(uint64_t* __restrict__ t, const uint64_t* __restrict__ inputs, uint32_t log_n) {
  const uint32_t n = 1u << log_n;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t* in = inputs + (uint64_t)i * 9;
  const word256::Head h(in[0]);
  // a padding row ignores its operand words and its exposed bit: it is the all-zero row with z = 1
  const U256 zero{0, 0, 0, 0};
  const U256 x = word256::operand<0>(in, h.live), y = word256::operand<1>(in, h.live);
  const bool sx = x.d >> 63, sy = y.d >> 63;
  const U256 ax = word256::magnitude(x), ay = word256::magnitude(y);
  const bool y_zero = word256::is_zero(y);
  const auto [q, r, d] = word256::divide(ax, ay, y_zero);
  // the quotient rounds toward zero and the remainder has the sign of x; -0 = 0 comes out of the negation by itself
  const bool neg = h.op_a ? sx != sy : h.op_b & sx;
  const U256 m = y_zero ? zero : h.op_a ? q : r;  // (a padding row has y = 0)
  const U256 res = neg ? word256::negate(m) : m;

  const Row row{t + i, n};
  row.put_head(sd::SHARED, h, y, y_zero);
  row.put(sd::COL_NEG, neg);
  uint64_t carry = 0;
  uint32_t borrow = 0;
  Chains chains{0, 0, 0};
  store_limbs<0>(row, x, y, ax, ay, q, r, d, m, res, carry, borrow, chains, sx, sy, neg, y_zero);
}

}  // namespace

extern "C" {

int bp_arithmetic_sdiv_layout(uint32_t* out, size_t n_words) { return word256::layout_entry("bp_arithmetic_sdiv_layout", sd::LAYOUT, out, n_words); }

int bp_arithmetic_sdiv_trace(const uint64_t* d_inputs, uint32_t log_n, uint64_t* d_trace_out, void* stream) try {
  return word256::trace_entry("bp_arithmetic_sdiv_trace", arithmetic_sdiv_trace_kernel, d_inputs, log_n, d_trace_out, stream);
}
BPG_ABI_CATCH("bp_arithmetic_sdiv_trace")

}  // extern "C"
