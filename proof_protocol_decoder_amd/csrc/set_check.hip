// set_check.hip -- the device side of bp_check_table_set and bp_check_txn_witness (include/bpg.h): does a link balance, and if
// not, which rows unbalance it -- computed where the traces are, a handful of words back to the host.
//
// Keys.  A lane owns a row of one end of the link and computes the port's filter f and its tuple compressed by two
// fresh challenges, v_0 = sum_j beta_0^j t_j and v_1 = sum_j beta_1^j t_j (trailing zeros of a tuple drop out of both).
// A registered program's port unit is interpreted exactly as program_port_terms_kernel interprets it (prog::run_port into
// a PortAcc; registers in LDS [reg][lane], the code and the beta table read wave-uniformly: air_program_dev.cuh).  A
// built-in member's come from builtin_port_keys (air_check_dev.cuh): one pass over the filter and tuple that
// air::ctl::product_term reads (air::ctl::port_tuple), Keccak-f's input 23 rows up.
//
// Balance.  Rows with f != 0 insert into an open-addressed table in HBM keyed by v_0: a slot is claimed by ONE 64-bit
// compare-and-swap on its key word (empty = all ones, which is no canonical field element; 0 is a key like any other),
// then linear probing.  A slot accumulates S = sum of +-f and S_1 = sum of +-f v_1 (looking rows add, looked rows add the
// negation mod p) as 128-bit integers -- an atomic add on the low word, whose returned old value tells this adder, and
// only this adder, whether it carried into the high word -- and the minima of the looking (end, row) and the looked row
// with atomicMin.  Integer adds and minima commute: the result is a function of the inputs, whatever the launch order.
// NO lane ever waits for another lane: a lane that loses the compare-and-swap reads the winner's key from the value the
// instruction returned and moves on; there is no lock and no "wait until the other word is written".
// A slot balances iff S = 0 and S_1 = 0 (mod p).  Two distinct tuple values that collide in v_0 (about n_tuple N^2 / 2^64)
// share a slot: if both balance both sums are exactly zero, so a collision never raises a false alarm; a false pass needs
// sum f (v_1 - v_1') = 0 as well, a second independent 2^-64-sized event.
//
// Contention.  A range-check link sends few distinct values from many rows.  A wave first peels the contribution of its
// first kept lane: the lanes with the same (key, +-f, +-f v_1) are found with a ballot and added once, count times the
// value.  Every lane of a launched wave takes the ballots: a row past the table (a 2^5-row table is half a wave) is a
// lane that keeps nothing, not an absent lane.
//
// Scan.  One pass over the slots reduces the sums, counts the unbalanced slots and takes the link-wide minima.  (The
// rows with f != 0 on each side are counted in the key pass, one add of a ballot's population per wave: a slot holds
// sums of f, not row counts.  The same pass tests the filter where the port demands a bit and takes the smallest bad
// (end, row); the value at that row is fetched by a one-workgroup launch of the same kernel, only when there is one.)
#include <mutex>
#include <vector>
#include "air_check_dev.cuh"
#include "air_program.hpp"
#include "air_program_dev.cuh"
#include "common.hpp"
#include "set_check.hpp"

namespace {

using namespace bpg::chk;
using bpg::progdev::BetaTab;
using bpg::progdev::LdsRegs;
using bpg::progdev::lds_regs_of_lane;
namespace prog = bpg::air::prog;

constexpr unsigned long long EMPTY = ~0ull;

struct KeyArgs {
  const uint64_t *trace, *consts;
  uint64_t stride;
  uint32_t log_n, n_units, n_code, port;  // port: a program's port; a built-in's first product column of the port
  uint64_t pub[4], beta[2];
  unsigned long long *table, *res;
  uint64_t mask;       // slots - 1
  uint32_t shift;      // 64 - log2(slots)
  uint32_t looked, wants_bit;
  uint64_t end;
  uint64_t fetch_row;  // ~0: the balance; else only: res[SET_RES_BAD_VALUE] = f at that row
  uint32_t block0;     // the first workgroup's index (a fetch launches the row's workgroup alone)
};

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int lane) {
  return ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(v >> 32), lane) << 32) | (uint32_t)__shfl((int)(uint32_t)v, lane);
}
// w[0], w[1] += (lo, hi) as one 128-bit integer: whoever's add wraps the low word carries, and nobody else
__device__ __forceinline__ void add128(unsigned long long* w, uint64_t lo, uint64_t hi) {
  if (lo) {
    const unsigned long long old = atomicAdd(w, (unsigned long long)lo);
    hi += (old + lo < old);
  }
  if (hi) atomicAdd(w + 1, (unsigned long long)hi);
}

// Every lane of the wave gets here.  active: the lane owns a row of the table.
__device__ __forceinline__ void accumulate(const KeyArgs& a, bool active, uint64_t pos, uint64_t f, uint64_t v0, uint64_t v1) {
  if (a.fetch_row != ~0ull) {  // wave-uniform
    if (active && pos == a.fetch_row) a.res[bpg::SET_RES_BAD_VALUE] = f;
    return;
  }
  const uint32_t lane = threadIdx.x & 63;
  const unsigned long long loc = (a.end << bpg::SET_LOC_ROW_BITS) | pos;
  if (active && a.wants_bit && f > 1) atomicMin(a.res + bpg::SET_RES_BAD_FILTER, loc);
  const bool keep = active && f != 0;
  const unsigned long long kept = __ballot(keep);
  if (!kept) return;
  const int first = __ffsll(kept) - 1;
  if ((int)lane == first) atomicAdd(a.res + (a.looked ? bpg::SET_RES_N_LOOKED : bpg::SET_RES_N_LOOKING), (unsigned long long)__popcll(kept));
  const uint64_t fv = gl::mulc(f, v1);
  const uint64_t s = a.looked ? gl::negc(f) : f, s1 = a.looked ? gl::negc(fv) : fv;
  const bool same = keep && v0 == shfl64(v0, first) && s == shfl64(s, first) && s1 == shfl64(s1, first);
  const unsigned long long sames = __ballot(same);
  // (no ballot or shuffle below: the lanes part here)
  if (!keep || (same && (int)lane != __ffsll(sames) - 1)) return;
  const uint64_t count = same ? (uint64_t)__popcll(sames) : 1;  // the peeled lanes' first is their smallest row
  uint64_t h = (v0 * 0x9E3779B97F4A7C15ull) >> a.shift;
  unsigned long long* slot = nullptr;
  for (uint64_t tries = 0; tries <= a.mask; tries++) {
    unsigned long long* at = a.table + h * bpg::SET_SLOT_WORDS;
    const unsigned long long was = atomicCAS(at, EMPTY, (unsigned long long)v0);
    if (was == EMPTY || was == v0) {
      slot = at;
      break;
    }
    h = (h + 1) & a.mask;
  }
  if (!slot) {  // (the table has twice the rows: not reached)
    atomicAdd(a.res + bpg::SET_RES_OVERFLOW, 1ull);
    return;
  }
  add128(slot + 1, count * s, __umul64hi(count, s));
  add128(slot + 3, count * s1, __umul64hi(count, s1));
  if (a.looked) atomicMin(slot + 6, (unsigned long long)pos);
  else atomicMin(slot + 5, loc);
}

// the wave's rows: false when the whole wave lies past the table (it leaves together); a lane past the table in a
// wave that stays reads the last row and keeps nothing
__device__ __forceinline__ bool wave_rows(const KeyArgs& a, uint64_t n, bool* active, uint64_t* pos) {
  const uint64_t at = ((uint64_t)blockIdx.x + a.block0) * 256 + threadIdx.x;
  if ((at & ~63ull) >= n) return false;
  *active = at < n;
  *pos = *active ? at : n - 1;
  return true;
}

// grid = (ceil(n / 256)); dynamic LDS = n_regs * 2 KiB.  image: the program's device image (air_program.hpp).
__global__ void __launch_bounds__(256) set_keys_program_kernel(KeyArgs a, BetaTab bt, const uint64_t* __restrict__ image) {
  const uint64_t n = (uint64_t)1 << a.log_n;
  bool active;
  uint64_t pos;
  if (!wave_rows(a, n, &active, &pos)) return;
  const CheckRow row{a.trace, a.consts, a.stride, n, pos, (pos + 1) & (n - 1), gl::pow(gl::root(a.log_n), pos), a.pub};
  LdsRegs regs = lds_regs_of_lane();
  const uint64_t* __restrict__ code = image + a.n_units + 1;
  const uint64_t* __restrict__ port_off = code + a.n_code;
  prog::PortAcc<uint64_t> acc{bt.v, 0, 0, 0};
  prog::run_port<uint64_t>(code, (uint32_t)port_off[a.port], (uint32_t)port_off[a.port + 1], regs, row, acc);
  accumulate(a, active, pos, acc.f, acc.v0, acc.v1);
}

// grid = (ceil(n / 256)).  a.port: the port's first product column (first_product + 2 * port).
template <uint32_t AIR>
__global__ void __launch_bounds__(256) set_keys_builtin_kernel(KeyArgs a) {
  const uint64_t n = (uint64_t)1 << a.log_n;
  bool active;
  uint64_t pos;
  if (!wave_rows(a, n, &active, &pos)) return;
  uint64_t f, v0, v1;
  builtin_port_keys<AIR>(a.trace, a.stride, n, pos, a.port, a.beta[0], a.beta[1], &f, &v0, &v1);
  accumulate(a, active, pos, f, v0, v1);
}

// grid = (ceil(slots * 8 / 256)): every slot empty, the link's result words at their neutral values
__global__ void __launch_bounds__(256) set_clear_kernel(unsigned long long* table, uint64_t words, unsigned long long* res) {
  const uint64_t i = blockIdx.x * (uint64_t)256 + threadIdx.x;
  if (i < words) {
    const uint32_t w = (uint32_t)i & (bpg::SET_SLOT_WORDS - 1);
    table[i] = (w == 0 || w == 5 || w == 6) ? EMPTY : 0ull;
  }
  if (i < bpg::SET_RESULT_WORDS)
    res[i] = (i == bpg::SET_RES_MIN_LOOKING || i == bpg::SET_RES_MIN_LOOKED || i == bpg::SET_RES_BAD_FILTER) ? EMPTY : 0ull;
}

__device__ __forceinline__ uint64_t wave_min(uint64_t v) {
#pragma unroll
  for (int d = 32; d; d >>= 1) {
    const uint64_t o = shfl64(v, (int)((threadIdx.x & 63) ^ d));
    v = o < v ? o : v;
  }
  return v;
}
// grid = (ceil(slots / 256)): a lane owns a slot (every lane of a wave takes the ballot: slots is a multiple of 64 or
// the lanes past it hold nothing)
__global__ void __launch_bounds__(256) set_scan_kernel(const unsigned long long* table, uint64_t slots, unsigned long long* res) {
  const uint64_t i = blockIdx.x * (uint64_t)256 + threadIdx.x;
  bool off = false;
  uint64_t min_looking = EMPTY, min_looked = EMPTY;
  if (i < slots) {
    const unsigned long long* s = table + i * bpg::SET_SLOT_WORDS;
    if (s[0] != EMPTY) {
      off = gl::canon(gl::reduce128(s[1], s[2])) != 0 || gl::canon(gl::reduce128(s[3], s[4])) != 0;
      if (off) {
        min_looking = s[5];
        min_looked = s[6];
      }
    }
  }
  const unsigned long long offs = __ballot(off);
  if (!offs) return;
  min_looking = wave_min(min_looking);
  min_looked = wave_min(min_looked);
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(res + bpg::SET_RES_UNBALANCED, (unsigned long long)__popcll(offs));
    if (min_looking != EMPTY) atomicMin(res + bpg::SET_RES_MIN_LOOKING, (unsigned long long)min_looking);
    if (min_looked != EMPTY) atomicMin(res + bpg::SET_RES_MIN_LOOKED, (unsigned long long)min_looked);
  }
}

// A dynamic LDS allocation above 64 KiB has to be asked for before the launch (air_program.hip, allow_large_lds).
int allow_large_lds() {
  static std::mutex mu;
  static std::vector<int> done;
  int dev = 0;
  BPG_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(mu);
  for (int d : done)
    if (d == dev) return BP_OK;
  BPG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&set_keys_program_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(prog::MAX_REGS * 256 * 8)));
  done.push_back(dev);
  return BP_OK;
}

int launch_keys(const bpg::SetEnd& e, KeyArgs a, hipStream_t st) {
  const uint64_t n = (uint64_t)1 << e.log_n;
  a.trace = e.trace; a.consts = e.consts; a.stride = e.stride; a.log_n = e.log_n;
  a.end = e.end; a.looked = e.looked; a.wants_bit = e.wants_bit;
  for (int j = 0; j < 4; j++) a.pub[j] = e.pub[j];
  unsigned grid = bpg::ceil_div(n, 256);
  if (a.fetch_row != ~0ull) {
    a.block0 = (uint32_t)(a.fetch_row / 256);
    grid = 1;
  }
  if (prog::is_registered(e.air_id)) {
    const std::shared_ptr<const prog::Program> p = prog::find(e.air_id);
    if (!p || e.port >= p->n_ports) return bpg::fail(BP_ERR_INVALID_INPUT, "AIR program 0x%08x was unregistered", e.air_id);
    if (p->n_const && !e.consts) return bpg::fail(BP_ERR_INVALID_INPUT, "AIR program 0x%08x reads %u constant columns: pass them", e.air_id, p->n_const);
    if (int rc = allow_large_lds()) return rc;
    const uint64_t* d_image = nullptr;
    if (int rc = prog::device_image(p, &d_image)) return rc;
    a.n_units = p->n_units; a.n_code = p->n_code; a.port = e.port;
    BetaTab bt;
    const uint64_t ctl[4] = {a.beta[0], 0, a.beta[1], 0};
    prog::beta_powers(ctl, bt.v);
    set_keys_program_kernel<<<grid, 256, p->n_regs * 256 * 8, st>>>(a, bt, d_image);
  } else {
    if (e.air_id >= bpg::air::COUNT || !bpg::air::DESC[e.air_id].in_pair) return bpg::fail(BP_ERR_INVALID_INPUT, "no lookup is built for AIR %u", e.air_id);
    a.port = bpg::air::DESC[e.air_id].first_product + 2 * e.port;
    bpg::air::dispatch(e.air_id, [&](auto A) {
      if constexpr (bpg::air::DESC[A.value].in_pair) set_keys_builtin_kernel<A.value><<<grid, 256, 0, st>>>(a);
    });
  }
  BPG_LAUNCH_CHECK();
  return BP_OK;
}

}  // namespace

namespace bpg {

uint32_t set_check_log_slots(uint64_t rows) {
  uint32_t l = 6;  // at least a wave of slots
  while (((uint64_t)1 << l) < 2 * rows) l++;
  return l;
}

int launch_set_link(const SetEnd* ends, uint32_t n_ends, const uint64_t ctl[4], uint64_t* d_table, uint32_t log_slots, uint64_t* d_result,
                    hipStream_t st) {
  const uint64_t slots = (uint64_t)1 << log_slots, words = slots * SET_SLOT_WORDS;
  KeyArgs a{};
  a.table = reinterpret_cast<unsigned long long*>(d_table);
  a.res = reinterpret_cast<unsigned long long*>(d_result);
  a.mask = slots - 1;
  a.shift = 64 - log_slots;
  a.beta[0] = ctl[0]; a.beta[1] = ctl[2];
  a.fetch_row = ~0ull;
  set_clear_kernel<<<ceil_div(words, 256), 256, 0, st>>>(a.table, words, a.res);
  BPG_LAUNCH_CHECK();
  for (uint32_t m = 0; m < n_ends; m++)
    if (int rc = launch_keys(ends[m], a, st)) return rc;
  set_scan_kernel<<<ceil_div(slots, 256), 256, 0, st>>>(a.table, slots, a.res);
  BPG_LAUNCH_CHECK();
  return BP_OK;
}

int launch_set_filter_at(const SetEnd& e, uint64_t row, const uint64_t ctl[4], uint64_t* d_result, hipStream_t st) {
  KeyArgs a{};
  a.res = reinterpret_cast<unsigned long long*>(d_result);
  a.beta[0] = ctl[0]; a.beta[1] = ctl[2];
  a.fetch_row = row;
  return launch_keys(e, a, st);
}

}  // namespace bpg
