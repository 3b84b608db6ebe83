// air_check.hpp -- the AIR trace checker (air_check.hip: device pass, air_check.cpp: host pass and C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace bpg {

// One check of one trace on the trace domain (n = 2^log_n rows, x = w_n^i at row i).
struct CheckArgs {
  const uint64_t* trace;   // column-major, n_cols columns, column stride `stride`
  const uint64_t* consts;  // column-major, n_const columns, column stride n (AIRs 0 and 8), else NULL
  const uint64_t* apow;    // [2][T]: alpha_j^e, filled by launch_air_check
  uint64_t* partial;       // [wg_rows][2][n] when the units are spread over grid.y (or AIR 8), else NULL
  uint64_t* bitmap;        // [ceil(n / 64)]: bit i % 64 of word i / 64 = row i violates a constraint
  unsigned long long* count;  // violated rows (zeroed by launch_air_check)
  uint64_t stride, alpha0, alpha1;
  uint64_t pub[4];         // AIR 8's public inputs
  uint32_t air_id, log_n, n_cols, n_const, deg_pow;
  uint32_t T;              // the AIR's own constraints (the lookup part of the list is not checked)
  uint32_t n_units, units_per_wg, wg_rows;
};
// partial words (0: none) and the grid.y spreading for a check of `a` (fills n_units, units_per_wg, wg_rows)
uint64_t air_check_partial_words(CheckArgs& a);
int launch_air_check(const CheckArgs& a, hipStream_t st);
// air_program.hip: launch_air_check's row pass when a.air_id is a registered program (air_program.hpp)
int launch_air_check_program(const CheckArgs& a, dim3 grid, hipStream_t st);
// out[j * n_cols + c] = trace[c * stride + rows[j]], j < n_rows (d_rows on the device)
int launch_gather_rows(const uint64_t* trace, uint64_t stride, uint32_t n_cols, const uint32_t* d_rows, uint32_t n_rows,
                       uint64_t* out, hipStream_t st);

}  // namespace bpg
