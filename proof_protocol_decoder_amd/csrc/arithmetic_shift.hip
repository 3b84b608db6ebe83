// arithmetic_shift.hip -- the witness generator of the shift table (SHL, SHR and SAR on 256-bit words, one operation per
// row), the third table proven by a constraint PROGRAM shipped with the Python package (proof_protocol_decoder_amd/
// arithmetic_shift.py, registered at run time).  include/bpg.h states the entries and the input words, AIRS.md section 2
// ("Shift (a shipped program)") the columns and why the constraints are sound.
//
// The column map below exists a second time, in the Python program; bp_arithmetic_shift_layout hands this one out so
// that arithmetic_shift.register() can refuse to run when the two differ.  This table has no quotient, remainder or
// slack: of word256.cuh it uses the word, its limbs, the three-operation head, the operands, the stores and the entries.
#include "word256.cuh"

namespace {

namespace sh {
constexpr uint32_t LIMBS = 16, OFFSETS = 31;   // the limb offsets d = -15 .. 15 of the second one-hot: e_d at COL_E + 15 + d
constexpr uint32_t COL_IS_SHL = 0, COL_IS_SHR = 1, COL_IS_SAR = 2, COL_G = 3, COL_Z = 4, COL_INV = 5, COL_FILL = 6, COL_W = 7;
constexpr uint32_t COL_S = 8, COL_X = COL_S + LIMBS, COL_RES = COL_X + LIMBS, COL_Y = COL_RES + LIMBS;
constexpr uint32_t COL_L = COL_Y + LIMBS, COL_E = COL_L + LIMBS;
constexpr uint32_t COL_S_BITS = COL_E + OFFSETS, COL_X_BITS = COL_S_BITS + 256, COL_LO_BITS = COL_X_BITS + 256,
                   COL_HI_BITS = COL_LO_BITS + 256, N_COLS = COL_HI_BITS + 256;
constexpr uint32_t LAYOUT[] = {N_COLS, COL_IS_SHL, COL_IS_SHR, COL_IS_SAR, COL_G, COL_Z, COL_INV, COL_FILL, COL_W, COL_S, COL_X,
                               COL_RES, COL_Y, COL_L, COL_E, COL_S_BITS, COL_X_BITS, COL_LO_BITS, COL_HI_BITS};
static_assert(N_COLS == 1143, "AIRS.md section 2 lists 1143 columns");
}  // namespace sh

using word256::limb;
using word256::Row;
using word256::U256;

// w 2^b modulo 2^256, b < 256: whole registers first, then a funnel over the rest; no array, nothing indexed at run time
__device__ __forceinline__ U256 shift_left(const U256& w, uint32_t b) {
  const uint32_t q = b >> 6, r = b & 63;
  U256 t;
  t.d = q == 0 ? w.d : q == 1 ? w.c : q == 2 ? w.b : w.a;
  t.c = q == 0 ? w.c : q == 1 ? w.b : q == 2 ? w.a : 0;
  t.b = q == 0 ? w.b : q == 1 ? w.a : 0;
  t.a = q == 0 ? w.a : 0;
  if (r) {
    t.d = (t.d << r) | (t.c >> (64 - r));
    t.c = (t.c << r) | (t.b >> (64 - r));
    t.b = (t.b << r) | (t.a >> (64 - r));
    t.a = t.a << r;
  }
  return t;
}
// floor(w / 2^b), b < 256, the vacated bits filled from `fill` (all zeros or all ones)
__device__ __forceinline__ U256 shift_right(const U256& w, uint32_t b, uint64_t fill) {
  const uint32_t q = b >> 6, r = b & 63;
  U256 t;
  t.a = q == 0 ? w.a : q == 1 ? w.b : q == 2 ? w.c : w.d;
  t.b = q == 0 ? w.b : q == 1 ? w.c : q == 2 ? w.d : fill;
  t.c = q == 0 ? w.c : q == 1 ? w.d : fill;
  t.d = q == 0 ? w.d : fill;
  if (r) {
    t.a = (t.a >> r) | (t.b << (64 - r));
    t.b = (t.b >> r) | (t.c << (64 - r));
    t.c = (t.c >> r) | (t.d << (64 - r));
    t.d = (t.d >> r) | (fill << (64 - r));
  }
  return t;
}

// What a row stores for limb K: the limb of s, of x, of the bit-shifted word y and of the result, the bits of the first
// two, and the split x_K W = lo_K + 2^16 hi_K (W <= 2^16, so the product is below 2^32).
template <uint32_t K>
__device__ __forceinline__ void store_limbs(const Row& row, const U256& s, const U256& x, const U256& y, const U256& res, uint32_t w) {
  if constexpr (K < sh::LIMBS) {
    const uint32_t sk = limb<K>(s), xk = limb<K>(x), split = xk * w;
    row.put(sh::COL_S + K, sk);
    row.put(sh::COL_X + K, xk);
    row.put(sh::COL_RES + K, limb<K>(res));
    row.put(sh::COL_Y + K, limb<K>(y));
    row.put_bits(sh::COL_S_BITS + 16 * K, sk, 16);
    row.put_bits(sh::COL_X_BITS + 16 * K, xk, 16);
    row.put_bits(sh::COL_LO_BITS + 16 * K, split & 0xFFFFu, 16);
    row.put_bits(sh::COL_HI_BITS + 16 * K, split >> 16, 16);
    store_limbs<K + 1>(row, s, x, y, res, w);
  }
}

// One operation per row, one lane per row.  inputs: [row][9] (include/bpg.h).  The lane shifts x by the low four bits of
// s (the word y the constraints split limb by limb), then y by whole limbs, bits 4 .. 7 of s; a count of 256 or more
// leaves only the fill.  Stores are column-major.
__global__ void __launch_bounds__(256)
arithmetic_shift_trace_kernel(uint64_t* __restrict__ t, const uint64_t* __restrict__ inputs, uint32_t log_n) {
  const uint32_t n = 1u << log_n;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t* in = inputs + (uint64_t)i * 9;
  const word256::Head3 h(in[0]);
  const bool is_shl = h.op_a, right = h.op_b | h.op_c;
  // a padding row ignores its operand words and its exposed bit: s = x = 0, so z = l_0 = e_0 = 1 and W = 0
  const U256 s = word256::operand<0>(in, h.live), x = word256::operand<1>(in, h.live);
  const uint32_t s0 = limb<0>(s);
  const uint32_t high = word256::limb_sum(s) - (s0 & 0xFFu);   // the limbs 1 .. 15 and 2^8 times bits 8 .. 15 of limb 0
  const uint32_t sum = high - s0 + (s0 & 0xFFu) + (s0 >> 8);    // T: the limbs 1 .. 15 plus the value of bits 8 .. 15
  const bool small = high == 0;                                 // s < 256
  const uint32_t low = s0 & 15u, limbs = (s0 >> 4) & 15u;
  const bool fill = h.op_c & (bool)(x.d >> 63);
  const uint64_t fill_word = fill ? ~(uint64_t)0 : 0;
  const uint32_t w = is_shl ? 1u << low : right ? 1u << (16 - low) : 0u;

  const U256 y = is_shl ? shift_left(x, low) : right ? shift_right(x, low, fill_word) : U256{0, 0, 0, 0};
  const U256 moved = is_shl ? shift_left(y, 16 * limbs) : shift_right(y, 16 * limbs, fill_word);
  const U256 res = small ? moved : U256{fill_word, fill_word, fill_word, fill_word};

  const Row row{t + i, n};
  row.put(sh::COL_IS_SHL, h.op_a);
  row.put(sh::COL_IS_SHR, h.op_b);
  row.put(sh::COL_IS_SAR, h.op_c);
  row.put(sh::COL_G, h.g());
  row.put(sh::COL_Z, small);
  row.put(sh::COL_INV, small ? 0 : gl::inv((uint64_t)sum));
  row.put(sh::COL_FILL, fill);
  row.put(sh::COL_W, w);
  row.put_bits(sh::COL_L, 1u << low, sh::LIMBS);
  // e_d, d = +limbs under SHL, -limbs under SHR and SAR, 0 on a padding row; no e at all when s >= 256
  row.put_bits(sh::COL_E, small ? 1u << (is_shl ? 15 + limbs : 15 - limbs) : 0u, sh::OFFSETS);
  store_limbs<0>(row, s, x, y, res, w);
}

}  // namespace

extern "C" {

int bp_arithmetic_shift_layout(uint32_t* out, size_t n_words) { return word256::layout_entry("bp_arithmetic_shift_layout", sh::LAYOUT, out, n_words); }

int bp_arithmetic_shift_trace(const uint64_t* d_inputs, uint32_t log_n, uint64_t* d_trace_out, void* stream) try {
  return word256::trace_entry("bp_arithmetic_shift_trace", arithmetic_shift_trace_kernel, d_inputs, log_n, d_trace_out, stream);
}
BPG_ABI_CATCH("bp_arithmetic_shift_trace")

}  // extern "C"
