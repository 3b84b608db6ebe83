// air_program.hip -- the device instantiation of the program interpreter (air_program.hpp): K5 on the LDE coset and the
// trace checker's row pass for REGISTERED AIRs, beside quotient_air_kernel (stark_kernels.hip) and air_check_kernel
// (air_check.hip), with their row accessors, consumers, alpha-power tables and partial-sum paths (quotient_dev.cuh,
// air_check_dev.cuh): the fold of a program is the built-in kernels' fold.
//
// A lane owns one point; the code is read wave-uniformly (scalar loads: pc never depends on the lane, nothing is
// decoded per lane) and every branch of the interpreter is a scalar branch.
//
// The register file.  A register numbered at run time cannot be a VGPR (the compiler would put the array in scratch), so
// the program's registers live in LDS as [reg][lane]: register r of lane l at word r * 256 + l -- consecutive lanes,
// 8 bytes each, conflict-free ds_read_b64 / ds_write_b64, and no barrier anywhere: a lane only ever touches its own
// column.  A register is 2 KiB of the workgroup's LDS; the dynamic allocation is sized from the program's n_regs, so
// a program of 10 registers (20 KiB) keeps seven workgroups on a CU and one of 64 (128 KiB, the validator's limit) one.
// The value an instruction has just written also stays in a VGPR (`acc`): an operand that names the register written
// last is read from there, which takes half the LDS reads out of the chains  v = v + v, v = v + b, e = e - c  these
// programs mostly are.
//
// Lookup ports ("BPGAIRP2").  A port unit is one more unit of the same loop whose `port` words feed a PortAcc (the filter
// and the tuple compressed by both challenge sets: 6 VGPRs) instead of the fold; the slot of a `port` word is wave-uniform,
// so the beta-power table is read like the code, with scalar loads.  K5 then hands the port's five constraints to the
// same DevEmit (prog::port_constraints).  The witness of a port's two product columns is program_port_terms_kernel (the
// terms, a lane per trace row) followed by aux_suffix_product_kernel in the form AIR 8 uses (stark_kernels.hip).
//
// Log ports ("BPGAIRP3").  The kinds travel in the image behind the port offsets and are read like them, with scalar
// loads: which of the two constraint forms a port unit ends in is a wave-uniform branch.  The kernels of a program with a
// log port are instantiations of their own (LOG): a program without one runs the code it ran before log ports existed.
// The witness of a log port is h_c = f / d_c in its two columns (one inversion per lane for both challenge sets) followed
// by the suffix SUM of port_running_columns_kernel (stark_kernels.hip).
#include <mutex>
#include "air_check_dev.cuh"
#include "air_program.hpp"
#include "air_program_dev.cuh"
#include "common.hpp"
#include "quotient_dev.cuh"

namespace {

using namespace bpg::k5;
using namespace bpg::chk;
namespace prog = bpg::air::prog;
using bpg::progdev::BetaTab;
using bpg::progdev::LdsRegs;
using bpg::progdev::lds_regs_of_lane;

// image: the program's unit offsets (n_air_units + 1 words), then its code (prog::Program::image).
// grid = (rows / 256, workgroup rows, proofs) as quotient_air_kernel's; dynamic LDS = n_regs * 2 KiB.
// n_code: the program's code words; the port units' offsets (n_ports + 1 words) follow them in the image.
// PORTS: the program has lookup ports; without them the kernel is the one it was before ports existed.
// LOG: one of them is a log port; the kinds (n_ports words) follow the port units' offsets in the image.
template <bool PORTS, bool LOG = false>
__global__ void __launch_bounds__(256) quotient_program_kernel(bpg::ArgPtr<bpg::QuotArgs> args, const uint64_t* __restrict__ image,
                                                               uint32_t n_code) {
  BPG_ARG_BATCH(bpg::QuotArgs, args);
  if (gridDim.x * gridDim.y * gridDim.z <= 64) __builtin_amdgcn_s_setprio(3);  // small launch = latency-critical: issue first
  const bpg::QuotArgs& q = batch[blockIdx.z];
  const uint64_t rows = (uint64_t)1 << (q.log_n + q.rate_bits);
  const uint64_t pos = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (pos >= rows) return;
  const uint32_t n = 1u << q.log_n;
  const uint32_t t = (uint32_t)(pos >> q.log_n), m = (uint32_t)(pos & (n - 1));
  DevEmit out{q.apow, q.n_constraints, row_point(q, t, m),
              {gl::dot_zero(), gl::dot_zero(), gl::dot_zero(), gl::dot_zero()}, 0, 0, false};
  DevRow row{q.trace_lde, q.aux_lde, q.const_lde, q.trace_stride, q.aux_stride, q.const_stride, pos,
             ((uint64_t)t << q.log_n) | ((m + 1) & (n - 1)), out.rp.x, q.ctl.pub};
  LdsRegs regs = lds_regs_of_lane();
  const uint64_t* __restrict__ code = image + q.n_air_units + 1;
  const uint32_t n_units = q.n_air_units + q.n_ctl_units;
  const uint32_t u0 = blockIdx.y * q.units_per_wg, u1 = min(u0 + q.units_per_wg, n_units);
#pragma unroll 1
  for (uint32_t u = u0; u < u1; u++) {
    if (u < q.n_air_units) {
      prog::run<uint64_t>(code, (uint32_t)image[u], (uint32_t)image[u + 1], regs, row, out);
    } else if constexpr (PORTS) {
      const uint32_t l = u - q.n_air_units;
      const uint64_t* __restrict__ port_off = code + n_code;
      prog::PortAcc<uint64_t> acc{q.apow + 2 * (size_t)q.n_constraints + 48, 0, 0, 0};
      prog::run_port<uint64_t>(code, (uint32_t)port_off[l], (uint32_t)port_off[l + 1], regs, row, acc);
      const uint32_t base = q.n_air_constraints + prog::PORT_CONSTRAINTS * l;
      uint32_t kind = prog::PORT_PRODUCT;
      if constexpr (LOG) kind = (uint32_t)port_off[q.n_ports + 1 + l];
      if (LOG && kind != prog::PORT_PRODUCT) prog::log_port_constraints<uint64_t>(base, l, kind, q.ctl.v, acc, row, out);
      else prog::port_constraints<uint64_t>(base, l, q.ctl.v, acc, row, out);
    } else {
      // "a table no lookup is built for": the one constant running product AIR 4 and AIR 7 have
      const bpg::air::Shape cs{bpg::air::ARITHMETIC, q.n_cols, q.n_const, q.deg_pow};
      bpg::air::ctl::eval<uint64_t>(cs, q.n_air_constraints, 0, q.n_aux, q.ctl.v, row, out);
    }
  }
  const uint64_t r0 = out.result(0), r1 = out.result(1);
  if (gridDim.y == 1) {
    const uint64_t zh_inv = q.apow[2 * (size_t)q.n_constraints + 32 + t];
    q.qvals[pos] = gl::mulc(r0, zh_inv);
    q.qvals[rows + pos] = gl::mulc(r1, zh_inv);
  } else {
    q.partial[((uint64_t)blockIdx.y * 2) * rows + pos] = r0;
    q.partial[((uint64_t)blockIdx.y * 2 + 1) * rows + pos] = r1;
  }
}

// grid = (ceil(n / 256), wg_rows) as air_check_kernel's; dynamic LDS = n_regs * 2 KiB.
__global__ void __launch_bounds__(256) air_check_program_kernel(bpg::CheckArgs a, const uint64_t* __restrict__ image) {
  const uint64_t n = (uint64_t)1 << a.log_n;
  const uint64_t pos = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  uint64_t r0 = 0, r1 = 0;
  if (pos < n) {
    CheckEmit out = check_emit(a, pos);
    const CheckRow row = check_row(a, pos, true);
    LdsRegs regs = lds_regs_of_lane();
    const uint64_t* __restrict__ code = image + a.n_units + 1;
    const uint32_t u0 = blockIdx.y * a.units_per_wg, u1 = min(u0 + a.units_per_wg, a.n_units);
#pragma unroll 1
    for (uint32_t u = u0; u < u1; u++) prog::run<uint64_t>(code, (uint32_t)image[u], (uint32_t)image[u + 1], regs, row, out);
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

// beta_c^j, j < 128, c < 2, behind the per-coset words of every proof's alpha-power table.  One workgroup of 256 lanes
// per proof of the batch.
__global__ void __launch_bounds__(256) beta_table_kernel(bpg::ArgPtr<bpg::QuotArgs> args) {
  BPG_ARG_BATCH(bpg::QuotArgs, args);
  const bpg::QuotArgs& q = batch[blockIdx.x];
  const uint32_t t = threadIdx.x;
  const_cast<uint64_t*>(q.apow)[2 * (size_t)q.n_constraints + 48 + t] = gl::pow(q.ctl.v[t >> 7 ? 2 : 0], t & (prog::MAX_TUPLE - 1));
}

// The terms of a program's ports on the trace domain: a lane owns a trace row (the checker's row accessor: nxt wraps,
// x = w^i), runs the port units of its workgroup row and writes term_0, term_1 of each into the port's two auxiliary
// columns, where aux_suffix_product_kernel multiplies them up.  The beta powers travel as a kernel argument (2 KiB,
// read wave-uniformly).  grid = (ceil(n / 256), n_ports); dynamic LDS = n_regs * 2 KiB.
// LOG (a program with a log port): a log port's columns get h_c = f / d_c, d_c = gamma_c + v_c, which the scan then sums.
// Both inverses come from one inversion of d_0 d_1.  A zero denominator is taken as 1 before the product, so it spoils
// neither the other challenge set's inverse nor anything else: with f = 0 the row contributes 0 either way, and with
// f != 0 (a pole: the sum has no value) the row is reported through `pole` -- [n_ports][2] words, the smallest such row
// per port and challenge set -- and the caller fails.
struct PortTermsArgs {
  const uint64_t *trace, *consts;
  uint64_t* aux;  // [2 * n_ports][n]
  uint64_t stride;
  uint32_t log_n, n_units, n_code, n_ports;
  uint64_t ctl[4], pub[4];
  unsigned long long* pole;  // LOG only
};
template <bool LOG>
__global__ void __launch_bounds__(256) program_port_terms_kernel(PortTermsArgs a, BetaTab bt, const uint64_t* __restrict__ image) {
  const uint64_t n = (uint64_t)1 << a.log_n;
  const uint64_t pos = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (pos >= n) return;
  const CheckRow row{a.trace, a.consts, a.stride, n, pos, (pos + 1) & (n - 1), gl::pow(gl::root(a.log_n), pos), a.pub};
  LdsRegs regs = lds_regs_of_lane();
  const uint64_t* __restrict__ code = image + a.n_units + 1;
  const uint64_t* __restrict__ port_off = code + a.n_code;
  const uint32_t l = blockIdx.y;
  prog::PortAcc<uint64_t> acc{bt.v, 0, 0, 0};
  prog::run_port<uint64_t>(code, (uint32_t)port_off[l], (uint32_t)port_off[l + 1], regs, row, acc);
  if constexpr (LOG) {
    if (port_off[a.n_ports + 1 + l] != prog::PORT_PRODUCT) {  // wave-uniform
      const uint64_t d0 = acc.denom(0, a.ctl), d1 = acc.denom(1, a.ctl);
      const uint64_t e0 = d0 ? d0 : 1, e1 = d1 ? d1 : 1;
      const uint64_t fi = gl::mulc(acc.f, gl::inv(gl::mulc(e0, e1)));  // f / (d_0 d_1)
      a.aux[(uint64_t)(2 * l) * n + pos] = d0 ? gl::mulc(fi, e1) : 0;
      a.aux[(uint64_t)(2 * l + 1) * n + pos] = d1 ? gl::mulc(fi, e0) : 0;
      if (acc.f != 0) {
        if (d0 == 0) atomicMin(a.pole + 2 * l, (unsigned long long)pos);
        if (d1 == 0) atomicMin(a.pole + 2 * l + 1, (unsigned long long)pos);
      }
      return;
    }
  }
  a.aux[(uint64_t)(2 * l) * n + pos] = acc.term(0, a.ctl);
  a.aux[(uint64_t)(2 * l + 1) * n + pos] = acc.term(1, a.ctl);
}

// A dynamic LDS allocation above 64 KiB has to be asked for before the launch: once per device and kernel, for the
// validator's limit (prog::MAX_REGS registers), so every registered program fits.
int allow_large_lds() {
  static std::mutex mu;
  static std::vector<int> done;
  int dev = 0;
  BPG_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(mu);
  for (int d : done)
    if (d == dev) return BP_OK;
  const int bytes = (int)(prog::MAX_REGS * 256 * 8);
  BPG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&quotient_program_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  BPG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&quotient_program_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  BPG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&quotient_program_kernel<true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  BPG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&air_check_program_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  BPG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&program_port_terms_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  BPG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&program_port_terms_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  done.push_back(dev);
  return BP_OK;
}

int program_of(uint32_t air_id, uint32_t n_units, std::shared_ptr<const prog::Program>* p, const uint64_t** d_image) {
  *p = prog::find(air_id);
  if (!*p) return bpg::fail(BP_ERR_INVALID_INPUT, "AIR program 0x%08x was unregistered", air_id);
  if ((*p)->n_units != n_units) return bpg::fail(BP_ERR_INVALID_INPUT, "AIR program 0x%08x: the launch was sized for another program", air_id);
  if (int rc = allow_large_lds()) return rc;
  return prog::device_image(*p, d_image);
}

}  // namespace

namespace bpg {

// The evaluation launch of launch_quotient (stark_kernels.hip) for a registered id: same grid, same argument blocks.
int launch_quotient_program(const QuotArgs* qb, const QuotArgs& q, dim3 grid, KernelTimer& kt, hipStream_t st) {
  std::shared_ptr<const prog::Program> p;
  const uint64_t* d_image = nullptr;
  if (int rc = program_of(q.air_id, q.n_air_units, &p, &d_image)) return rc;
  if (q.n_ports != p->n_ports) return bpg::fail(BP_ERR_INVALID_INPUT, "AIR program 0x%08x: the launch was sized for another program", q.air_id);
  if (p->log_ports()) BPG_LAUNCH_TIMED(kt, HIP_KERNEL_NAME(quotient_program_kernel<true, true>), grid, 256, p->n_regs * 256 * 8, st, arg_ptr(qb), d_image, p->n_code);
  else if (q.n_ports) BPG_LAUNCH_TIMED(kt, quotient_program_kernel<true>, grid, 256, p->n_regs * 256 * 8, st, arg_ptr(qb), d_image, p->n_code);
  else BPG_LAUNCH_TIMED(kt, quotient_program_kernel<false>, grid, 256, p->n_regs * 256 * 8, st, arg_ptr(qb), d_image, p->n_code);
  return BP_OK;
}

// The beta powers of every proof of a batch, beside its alpha powers: launch_quotient issues this with the alpha tables,
// before the evaluation launch and its timer.
int launch_beta_tables(const QuotArgs* qb, uint32_t batch, hipStream_t st) {
  beta_table_kernel<<<batch, 256, 0, st>>>(arg_ptr(qb));
  BPG_LAUNCH_CHECK();
  return BP_OK;
}

int launch_port_terms(const AuxArgs& a, uint32_t air_id, uint32_t log_n, uint64_t trace_stride, uint64_t* d_pole, hipStream_t st) {
  std::shared_ptr<const prog::Program> p = prog::find(air_id);
  if (!p || !p->n_ports) return bpg::fail(BP_ERR_INVALID_INPUT, "air_id 0x%08x is no registered program with lookup ports", air_id);
  const uint64_t* d_image = nullptr;
  if (int rc = program_of(air_id, p->n_units, &p, &d_image)) return rc;
  if (p->n_const && !a.consts) return bpg::fail(BP_ERR_INVALID_INPUT, "AIR program 0x%08x reads %u constant columns: pass them", air_id, p->n_const);
  if (p->log_ports() && !d_pole) return bpg::fail(BP_ERR_INVALID_INPUT, "AIR program 0x%08x has log ports: the launch needs the pole words", air_id);
  PortTermsArgs pa{a.trace, a.consts, a.aux, trace_stride, log_n, p->n_units, p->n_code, p->n_ports, {}, {}, reinterpret_cast<unsigned long long*>(d_pole)};
  for (int i = 0; i < 4; i++) { pa.ctl[i] = a.ctl.v[i]; pa.pub[i] = a.ctl.pub[i]; }
  BetaTab bt;
  prog::beta_powers(a.ctl.v, bt.v);
  const dim3 grid((unsigned)((((uint64_t)1 << log_n) + 255) / 256), p->n_ports);
  if (p->log_ports()) program_port_terms_kernel<true><<<grid, 256, p->n_regs * 256 * 8, st>>>(pa, bt, d_image);
  else program_port_terms_kernel<false><<<grid, 256, p->n_regs * 256 * 8, st>>>(pa, bt, d_image);
  BPG_LAUNCH_CHECK();
  return BP_OK;
}

// The row pass of launch_air_check (air_check.hip) for a registered id.
int launch_air_check_program(const CheckArgs& a, dim3 grid, hipStream_t st) {
  std::shared_ptr<const prog::Program> p;
  const uint64_t* d_image = nullptr;
  if (int rc = program_of(a.air_id, a.n_units, &p, &d_image)) return rc;
  air_check_program_kernel<<<grid, 256, p->n_regs * 256 * 8, st>>>(a, d_image);
  return BP_OK;
}

}  // namespace bpg
