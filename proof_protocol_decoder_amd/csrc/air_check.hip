// air_check.hip -- the AIR trace checker's device pass: air.hpp's evaluators instantiated a third time, on the TRACE
// domain (the prover's K5 evaluates them on the LDE coset, the verifier over the extension field at zeta).
//
// A lane owns row i of the n = 2^log_n-row trace: loc = row i, nxt = row (i + 1) mod n, x = w_n^i.  The constraints are
// folded with two fresh challenges exactly as K5's consumer does (alpha-power table, gl::DotAcc), with the selectors of
// the trace domain: all-rows constraints everywhere, transition constraints on every row but n - 1, first-row ones on
// row 0, last-row ones on row n - 1.  A row is violated when either fold is non-zero.  Only a fold is a statement:
// units emit partial sums of one constraint several times (AIRS.md section 1), so no single emission is tested.
// What the units emit past the AIR's own list (the lookup shares of the logic and sponge tables, AIR 8's copy
// constraints) is dropped, and the auxiliary columns read as zero: the AIR's own values do not depend on them.
// Output: one bitmap word per 64 rows, written by the wave that owns them (__ballot), and the violated-row count.
// Which constraint a violated row breaks is the host's question (air_check.cpp).
#include <algorithm>
#include "air_check.hpp"
#include "common.hpp"
#include "gl.hpp"
#include "air.hpp"
#include "air_check_dev.cuh"
#include "air_program.hpp"

namespace {

using bpg::CheckArgs;
using namespace bpg::chk;

// grid = (ceil(n / 256), wg_rows): workgroup row y evaluates units [y * units_per_wg, ...) of the AIR's list (AIR 8:
// its ten chunk units; the Poseidon gate is air_check_plonk_hash_kernel's).  One workgroup row: the row's fold is
// complete and tested here; several: the partial folds go to `partial` and air_check_reduce_kernel tests their sum.
template <uint32_t AIR>
__global__ void __launch_bounds__(256) air_check_kernel(CheckArgs a) {
  const uint64_t n = (uint64_t)1 << a.log_n;
  const uint64_t pos = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  uint64_t r0 = 0, r1 = 0;
  if (pos < n) {
    CheckEmit out = check_emit(a, pos);
    const CheckRow row = check_row(a, pos, AIR == bpg::air::PLONK);
    const bpg::air::Shape shape{AIR, a.n_cols, a.n_const, a.deg_pow};
    const uint64_t ctl[4] = {0, 0, 0, 0};  // (only the dropped lookup shares read them)
    const uint32_t u0 = blockIdx.y * a.units_per_wg, u1 = min(u0 + a.units_per_wg, a.n_units);
#pragma unroll 1
    for (uint32_t u = u0; u < u1; u++) {
      bpg::air::eval_unit_of<AIR, uint64_t>(shape, u, a.T, ctl, row, out);
    }
    r0 = out.result(0);
    r1 = out.result(1);
  }
  if (a.partial) {
    if (pos < n) {
      a.partial[((uint64_t)blockIdx.y * 2) * n + pos] = r0;
      a.partial[((uint64_t)blockIdx.y * 2 + 1) * n + pos] = r1;
    }
    return;
  }
  flag_rows(a, pos, (r0 | r1) != 0);
}
// AIR 8's Poseidon gate (K5 keeps it in a kernel of its own for the register budget, and so does the checker): the bare
// differences folded, times q_hash, into partial row `wg_row`.   grid = (ceil(n / 256))
__global__ void __launch_bounds__(256) air_check_plonk_hash_kernel(CheckArgs a, uint32_t wg_row) {
  const uint64_t n = (uint64_t)1 << a.log_n;
  const uint64_t pos = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (pos >= n) return;
  CheckEmit out = check_emit(a, pos);
  const CheckRow row = check_row(a, pos, false);
  bpg::air::plonk::eval_hash_unit<uint64_t, CheckRow, CheckEmit, false>(row, out);
  const uint64_t qh = row.cst(bpg::air::plonk::CST_HASH);
  a.partial[((uint64_t)wg_row * 2) * n + pos] = gl::mulc(out.result(0), qh);
  a.partial[((uint64_t)wg_row * 2 + 1) * n + pos] = gl::mulc(out.result(1), qh);
}
// the sum of the partial folds, tested.   grid = (ceil(n / 256))
__global__ void __launch_bounds__(256) air_check_reduce_kernel(CheckArgs a, uint32_t n_rows) {
  const uint64_t n = (uint64_t)1 << a.log_n;
  const uint64_t pos = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  uint64_t r0 = 0, r1 = 0;
  if (pos < n)
    for (uint32_t c = 0; c < n_rows; c++) {
      r0 = gl::addc(r0, a.partial[((uint64_t)c * 2) * n + pos]);
      r1 = gl::addc(r1, a.partial[((uint64_t)c * 2 + 1) * n + pos]);
    }
  flag_rows(a, pos, (r0 | r1) != 0);
}
// apow[j * T + e] = alpha_j^e.   grid = (ceil(T / 256), 2)
__global__ void __launch_bounds__(256) air_check_alpha_kernel(uint64_t* apow, uint32_t T, uint64_t a0, uint64_t a1) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= T) return;
  apow[(uint64_t)blockIdx.y * T + e] = gl::pow(blockIdx.y ? a1 : a0, e);
}
// out[j * n_cols + c] = trace[c * stride + rows[j]].   grid = (ceil(n_cols / 256), n_rows)
__global__ void __launch_bounds__(256) air_check_gather_kernel(const uint64_t* trace, uint64_t stride, uint32_t n_cols,
                                                               const uint32_t* rows, uint64_t* out) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cols) return;
  out[(uint64_t)blockIdx.y * n_cols + c] = trace[(uint64_t)c * stride + rows[blockIdx.y]];
}

}  // namespace

namespace bpg {

uint64_t air_check_partial_words(CheckArgs& a) {
  const air::Shape shape{a.air_id, a.n_cols, a.n_const, a.deg_pow};
  const bool plonk = a.air_id == air::PLONK;
  a.n_units = plonk ? air::plonk::N_UNITS - 1 : air::any_n_units(shape);  // (AIR 8's unit 10: the hash kernel)
  const uint64_t blocks = ceil_div((uint64_t)1 << a.log_n, 256);
  // a table of 512 workgroups or more fills the chip's 256 CUs alone: one pass; a shorter one spreads its units
  // over grid.y up to ~1024 workgroups, as K5 does
  if (blocks >= 512 || a.n_units == 1) {
    a.units_per_wg = a.n_units;
  } else {
    const uint32_t want = (uint32_t)std::min<uint64_t>(a.n_units, ceil_div(1024, blocks));
    a.units_per_wg = ceil_div(a.n_units, want);
  }
  a.wg_rows = ceil_div(a.n_units, a.units_per_wg);
  const uint32_t rows = a.wg_rows + (plonk ? 1 : 0);
  return rows > 1 ? 2 * ((uint64_t)rows << a.log_n) : 0;
}

int launch_air_check(const CheckArgs& a, hipStream_t st) {
  const uint64_t n = (uint64_t)1 << a.log_n;
  BPG_HIP(hipMemsetAsync(a.count, 0, sizeof(unsigned long long), st));
  air_check_alpha_kernel<<<dim3(ceil_div(a.T, 256), 2), 256, 0, st>>>(const_cast<uint64_t*>(a.apow), a.T, a.alpha0, a.alpha1);
  BPG_LAUNCH_CHECK();
  const dim3 g1(ceil_div(n, 256), a.wg_rows);
  if (air::prog::is_registered(a.air_id)) {
    if (int rc = launch_air_check_program(a, g1, st)) return rc;
  } else air::dispatch(a.air_id, [&](auto A) { air_check_kernel<A.value><<<g1, 256, 0, st>>>(a); });
  BPG_LAUNCH_CHECK();
  if (a.air_id == air::PLONK) {
    air_check_plonk_hash_kernel<<<ceil_div(n, 256), 256, 0, st>>>(a, a.wg_rows);
    BPG_LAUNCH_CHECK();
  }
  if (a.partial) {
    air_check_reduce_kernel<<<ceil_div(n, 256), 256, 0, st>>>(a, a.wg_rows + (a.air_id == air::PLONK ? 1 : 0));
    BPG_LAUNCH_CHECK();
  }
  return BP_OK;
}

int launch_gather_rows(const uint64_t* trace, uint64_t stride, uint32_t n_cols, const uint32_t* d_rows, uint32_t n_rows,
                       uint64_t* out, hipStream_t st) {
  if (!n_rows || !n_cols) return BP_OK;
  air_check_gather_kernel<<<dim3(ceil_div(n_cols, 256), n_rows), 256, 0, st>>>(trace, stride, n_cols, d_rows, out);
  BPG_LAUNCH_CHECK();
  return BP_OK;
}

}  // namespace bpg
