// arithmetic_exp.hip -- the witness generator of the exponentiation table (EXP on 256-bit words, one exponent bit per
// row), the fifth table proven by a constraint PROGRAM shipped with the Python package (proof_protocol_decoder_amd/
// arithmetic_exp.py, registered at run time) instead of a built-in AIR, and the first whose statement spans rows.
// include/bpg.h states the entries and the input words, AIRS.md section 2 ("Exponentiation (a shipped program)") the
// columns and why the constraints are sound.
//
// The column map below exists a second time, in the Python program; bp_arithmetic_exp_layout hands this one out so that
// arithmetic_exp.register() can refuse to run when the two differ.  What the table shares with the other four is in
// word256.cuh (the word, its limbs, the multiply modulo 2^256, a lane's row); this file keeps the map, the search for a
// row's operation, the replay of its earlier steps, the two products' carries and the kernel.
#include "word256.cuh"

namespace {

namespace ex {
constexpr uint32_t LIMBS = 16, CARRY_BITS = 20, MAX_STEPS = 255;
constexpr uint32_t COL_G = 0, COL_FIRST = 1, COL_LAST = 2;
constexpr uint32_t COL_P = 3, COL_E = COL_P + LIMBS, COL_RES = COL_E + LIMBS, COL_R = COL_RES + LIMBS, COL_OUT = COL_R + LIMBS;
constexpr uint32_t COL_P_BITS = COL_OUT + LIMBS, COL_R_BITS = COL_P_BITS + 256, COL_E_BITS = COL_R_BITS + 256,
                   COL_M_BITS = COL_E_BITS + 256, COL_S_BITS = COL_M_BITS + 256;
constexpr uint32_t COL_M_CARRY = COL_S_BITS + 256, COL_S_CARRY = COL_M_CARRY + LIMBS * CARRY_BITS,
                   N_COLS = COL_S_CARRY + LIMBS * CARRY_BITS;
constexpr uint32_t LAYOUT[] = {N_COLS, COL_G, COL_FIRST, COL_LAST, COL_P, COL_E, COL_RES, COL_R, COL_OUT, COL_P_BITS, COL_R_BITS,
                               COL_E_BITS, COL_M_BITS, COL_S_BITS, COL_M_CARRY, COL_S_CARRY, CARRY_BITS};
}  // namespace ex

using word256::limb;
using word256::mul_low;
using word256::Row;
using word256::U256;

// the chain's state on one row: the running square, the running result, the exponent still to consume
struct State {
  U256 p, r, e;
};

// the number of steps before an operation's last row: the position of the exponent's highest set bit, 0 for e < 2
__device__ __forceinline__ uint32_t steps_of(const U256& e) {
  if (e.d) return 255u - (uint32_t)__clzll(e.d);
  if (e.c) return 191u - (uint32_t)__clzll(e.c);
  if (e.b) return 127u - (uint32_t)__clzll(e.b);
  return e.a ? 63u - (uint32_t)__clzll(e.a) : 0u;
}

// one step of binary exponentiation from the least significant bit: a multiply on a 1 bit, a squaring, the bit consumed
__device__ __forceinline__ void step(State& s) {
  if (s.e.a & 1) s.r = mul_low(s.r, s.p);
  s.p = mul_low(s.p, s.p);
  s.e.a = (s.e.a >> 1) | (s.e.b << 63);
  s.e.b = (s.e.b >> 1) | (s.e.c << 63);
  s.e.c = (s.e.c >> 1) | (s.e.d << 63);
  s.e.d >>= 1;
}

// what a row stores for limb K of p, e, res, r, out, m, s, and the carries out of column K of r p and of p p: column +
// carry in = limb + 2^16 carry out, below 2^37, so a carry is below 2^21 and on an honest row below 2^20 (AIRS.md)
template <uint32_t K>
__device__ __forceinline__ void store_limbs(const Row& row, const State& s, const U256& res, const U256& out, const U256& m,
                                            const U256& sq, uint64_t& carry_m, uint64_t& carry_s) {
  if constexpr (K < ex::LIMBS) {
    const uint32_t pk = limb<K>(s.p), rk = limb<K>(s.r), ek = limb<K>(s.e), mk = limb<K>(m), sk = limb<K>(sq);
    row.put(ex::COL_P + K, pk);
    row.put(ex::COL_E + K, ek);
    row.put(ex::COL_RES + K, limb<K>(res));
    row.put(ex::COL_R + K, rk);
    row.put(ex::COL_OUT + K, limb<K>(out));
    row.put_bits(ex::COL_P_BITS + 16 * K, pk, 16);
    row.put_bits(ex::COL_R_BITS + 16 * K, rk, 16);
    row.put_bits(ex::COL_E_BITS + 16 * K, ek, 16);
    row.put_bits(ex::COL_M_BITS + 16 * K, mk, 16);
    row.put_bits(ex::COL_S_BITS + 16 * K, sk, 16);
    carry_m = (word256::conv<K>(s.r, s.p) + carry_m - mk) >> 16;
    carry_s = (word256::conv<K>(s.p, s.p) + carry_s - sk) >> 16;
    row.put_bits(ex::COL_M_CARRY + ex::CARRY_BITS * K, (uint32_t)carry_m, ex::CARRY_BITS);
    row.put_bits(ex::COL_S_CARRY + ex::CARRY_BITS * K, (uint32_t)carry_s, ex::CARRY_BITS);
    store_limbs<K + 1>(row, s, res, out, m, sq, carry_m, carry_s);
  }
}

// One lane per row.  ops: [n_ops][9], starts: [n_ops + 1], the exclusive prefix sum of the operations' rows (include/
// bpg.h).  The lane finds its operation by binary search in starts[0 .. n_ops - 1] -- it reads ops[op] with op < n_ops and
// starts[k] with k <= n_ops whatever the arrays hold --, replays the operation from its first row, keeps the state of its
// own row on the way and goes on to the last row for res; then derives every column.  The number of steps comes from the
// exponent, never from starts: a row past the operation's end repeats the end, and `last` is the state's own e < 2, so
// prefix sums that cut a chain short leave a trace the checker refuses.  The lane writes its own row and nothing else.
// Stores are column-major, so a wave's are contiguous.
__global__ void __launch_bounds__(256)
arithmetic_exp_trace_kernel(uint64_t* __restrict__ t, const uint64_t* __restrict__ ops, uint32_t n_ops,
                            const uint32_t* __restrict__ starts, uint32_t log_n) {
  const uint32_t n = 1u << log_n;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  // a padding row -- past the last operation, or of an operation whose op byte is not 1 -- is all zero except last = 1
  State s{{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
  uint32_t at = 0, first = 0, g = 0;
  if (n_ops != 0 && i < starts[n_ops]) {
    uint32_t lo = 0, hi = n_ops;  // the last op in [lo, hi) whose start is not above i
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (starts[mid] <= i) lo = mid;
      else hi = mid;
    }
    const uint64_t* in = ops + (uint64_t)lo * 9;
    const uint64_t w0 = in[0];
    if (((uint32_t)w0 & 0xFFu) == 1) {
      s.p = U256{in[1], in[2], in[3], in[4]};
      s.r = U256{1, 0, 0, 0};
      s.e = U256{in[5], in[6], in[7], in[8]};
      at = i - starts[lo];  // wraps where starts is wrong: clamped below
      first = at == 0;
      g = first & (uint32_t)(w0 >> 8) & 1u;
    }
  }
  uint32_t n_steps = steps_of(s.e);
  n_steps = n_steps < ex::MAX_STEPS ? n_steps : ex::MAX_STEPS;
  at = at < n_steps ? at : n_steps;

  State mine = s;
#pragma unroll 1
  for (uint32_t it = 0; it < n_steps; it++) {
    step(s);
    if (it + 1 == at) mine = s;
  }
  const U256 res = (s.e.a & 1) ? mul_low(s.r, s.p) : s.r;  // the last row's out

  const U256 m = mul_low(mine.r, mine.p), sq = mul_low(mine.p, mine.p);
  const bool bit = mine.e.a & 1;
  const U256 out = bit ? m : mine.r;
  const bool last = (mine.e.b | mine.e.c | mine.e.d) == 0 && mine.e.a < 2;

  const Row row{t + i, n};
  row.put(ex::COL_G, g);
  row.put(ex::COL_FIRST, first);
  row.put(ex::COL_LAST, last);
  uint64_t carry_m = 0, carry_s = 0;
  store_limbs<0>(row, mine, res, out, m, sq, carry_m, carry_s);
}

}  // namespace

extern "C" {

int bp_arithmetic_exp_layout(uint32_t* out, size_t n_words) { return word256::layout_entry("bp_arithmetic_exp_layout", ex::LAYOUT, out, n_words); }

int bp_arithmetic_exp_trace(const uint64_t* d_ops, uint32_t n_ops, const uint32_t* d_starts, uint32_t log_n, uint64_t* d_trace_out,
                            void* stream) try {
  const char* name = "bp_arithmetic_exp_trace";
  if (!d_trace_out) return bpg::fail(BP_ERR_INVALID_INPUT, "%s: null output", name);
  if (log_n < 4 || log_n > 26) return bpg::fail(BP_ERR_INVALID_INPUT, "%s: log_n out of range", name);
  if (n_ops > (uint64_t)1 << log_n) return bpg::fail(BP_ERR_INVALID_INPUT, "%s: %u operations in 2^%u rows", name, n_ops, log_n);
  if (n_ops && !d_ops) return bpg::fail(BP_ERR_INVALID_INPUT, "%s: null operations", name);
  if (n_ops && !d_starts) return bpg::fail(BP_ERR_INVALID_INPUT, "%s: null starts", name);
  arithmetic_exp_trace_kernel<<<bpg::ceil_div((uint64_t)1 << log_n, 256), 256, 0, bpg::as_stream(stream)>>>(d_trace_out, d_ops, n_ops,
                                                                                                         d_starts, log_n);
  BPG_LAUNCH_CHECK();
  return BP_OK;
}
BPG_ABI_CATCH("bp_arithmetic_exp_trace")

}  // extern "C"
