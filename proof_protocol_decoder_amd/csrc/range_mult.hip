// range_mult.hip -- bp_range_multiplicities (include/bpg.h): how often every value of [0, 2^log_range) occurs in the
// kept rows of some trace columns.  The counts are the filter column of the looked side of a range-check lookup (a
// kind-2 log port over the constant column 0 .. 2^log_range - 1, air_program.hpp), so they are made before the trace is
// committed, from the limb columns the looking ports send.
//
// A histogram.  grid = (row chunks, columns); a lane reads one value per step, consecutive lanes consecutive rows.
// While 2^log_range counters fit a workgroup's LDS (Tune::range_lds_log) the workgroup counts there (32-bit counters, LDS
// atomics) and adds its non-zero bins to d_mult at the end, one 64-bit atomic each; above that the lanes add to d_mult
// directly.  Either way a wave first peels the value of its first kept lane: the lanes that hold the same value are
// counted with a ballot and added once.  Limbs of real traces are heavily repeated (zero above all), and the all-equal
// input, which would otherwise serialise 64 atomics of every wave on one address, becomes one add per wave.  Integer
// adds only: the result does not depend on the order, the path or the knob.
#include "common.hpp"
#include "tune.hpp"

namespace {

struct RangeArgs {
  const uint64_t *values, *filter;
  unsigned long long *mult, *first_bad;
  uint64_t stride, n_rows, chunk;  // chunk: rows per workgroup, a multiple of 256
  uint32_t log_range;
};

template <bool IN_LDS>
__global__ void __launch_bounds__(256) range_multiplicities_kernel(RangeArgs a) {
  extern __shared__ uint32_t hist[];  // IN_LDS: 2^log_range counters
  const uint64_t bins = (uint64_t)1 << a.log_range;
  if constexpr (IN_LDS) {
    for (uint32_t b = threadIdx.x; b < bins; b += 256) hist[b] = 0;
    __syncthreads();
  }
  const uint32_t col = blockIdx.y, lane = threadIdx.x & 63;
  const uint64_t* __restrict__ v = a.values + (uint64_t)col * a.stride;
  const uint64_t begin = blockIdx.x * a.chunk, end = begin + a.chunk < a.n_rows ? begin + a.chunk : a.n_rows;
  auto add = [&](uint32_t bin, uint32_t count) {
    if constexpr (IN_LDS) atomicAdd(&hist[bin], count);
    else atomicAdd(a.mult + bin, (unsigned long long)count);
  };
  // every lane of a wave takes every step (the ballots below want whole waves): begin is a multiple of 256
  for (uint64_t base = begin; base < end; base += 256) {
    const uint64_t row = base + threadIdx.x;
    bool keep = row < end && (!a.filter || a.filter[row] != 0);
    const uint64_t x = keep ? v[row] : 0;
    if (keep && x >= bins) {
      atomicMin(a.first_bad, (unsigned long long)((uint64_t)col * a.n_rows + row));
      keep = false;
    }
    const uint64_t kept = __ballot(keep);
    if (!kept) continue;
    const uint32_t x0 = (uint32_t)__shfl((int)(uint32_t)x, __ffsll((unsigned long long)kept) - 1);
    const bool same = keep && (uint32_t)x == x0;
    const uint64_t sames = __ballot(same);
    if (same) {
      if (lane == (uint32_t)__ffsll((unsigned long long)sames) - 1) add(x0, (uint32_t)__popcll(sames));
    } else if (keep) {
      add((uint32_t)x, 1);
    }
  }
  if constexpr (IN_LDS) {
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < bins; b += 256) {
      const uint32_t c = hist[b];
      if (c) atomicAdd(a.mult + b, (unsigned long long)c);
    }
  }
}

}  // namespace

extern "C" int bp_range_multiplicities(const uint64_t* d_values, uint64_t stride, uint32_t n_cols, uint64_t n_rows, const uint64_t* d_filter,
                                       uint32_t log_range, uint64_t* d_mult, uint64_t* first_bad, void* stream) try {
  if (!d_values || !d_mult || !first_bad) return bpg::fail(BP_ERR_INVALID_INPUT, "bp_range_multiplicities: null argument");
  *first_bad = ~0ULL;
  if (log_range < 1 || log_range > 24) return bpg::fail(BP_ERR_INVALID_INPUT, "bp_range_multiplicities: log_range = %u is outside 1 .. 24", log_range);
  if (n_cols < 1 || n_cols > 65535 || n_rows < 1 || n_rows > ((uint64_t)1 << 40) || stride < n_rows)
    return bpg::fail(BP_ERR_INVALID_INPUT, "bp_range_multiplicities: %u columns (1 .. 65535) of %llu rows (1 .. 2^40), column stride %llu", n_cols,
                     (unsigned long long)n_rows, (unsigned long long)stride);
  hipStream_t st = bpg::as_stream(stream);
  // chunks of at least 4096 rows (a workgroup's flush of the LDS histogram is paid per chunk), at most 1024 per column;
  // a chunk stays below 2^32 rows, so a 32-bit LDS counter cannot wrap
  const uint64_t n_chunks = std::max<uint64_t>(1, std::min<uint64_t>(1024, n_rows / 4096));
  RangeArgs a{};
  a.values = d_values; a.filter = d_filter; a.mult = reinterpret_cast<unsigned long long*>(d_mult);
  a.stride = stride; a.n_rows = n_rows; a.log_range = log_range;
  a.chunk = ((n_rows + n_chunks - 1) / n_chunks + 255) / 256 * 256;
  const dim3 grid((unsigned)((n_rows + a.chunk - 1) / a.chunk), n_cols);
  BPG_HIP(hipMalloc(reinterpret_cast<void**>(&a.first_bad), 8));
  struct Free {
    void* p;
    ~Free() { (void)hipFree(p); }
  } free_it{a.first_bad};
  BPG_HIP(hipMemsetAsync(a.first_bad, 0xFF, 8, st));
  if ((int)log_range <= bpg::tune().range_lds_log.load())
    range_multiplicities_kernel<true><<<grid, 256, (size_t)4 << log_range, st>>>(a);
  else
    range_multiplicities_kernel<false><<<grid, 256, 0, st>>>(a);
  BPG_LAUNCH_CHECK();
  BPG_HIP(hipMemcpyAsync(first_bad, a.first_bad, 8, hipMemcpyDeviceToHost, st));
  BPG_HIP(hipStreamSynchronize(st));
  if (*first_bad != ~0ULL)
    return bpg::fail(BP_ERR_RANGE, "bp_range_multiplicities: column %llu, row %llu holds a value outside [0, 2^%u)",
                     (unsigned long long)(*first_bad / n_rows), (unsigned long long)(*first_bad % n_rows), log_range);
  return BP_OK;
}
BPG_ABI_CATCH("bp_range_multiplicities")
