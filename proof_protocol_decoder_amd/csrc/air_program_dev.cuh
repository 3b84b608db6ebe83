// air_program_dev.cuh -- the device pieces every kernel that interprets a registered program shares (air_program.hip: K5,
// the trace checker's row pass, the ports' witness; set_check.hip: the table-set pre-flight's keys): the register file in
// LDS and the beta-power table of the port units.
#pragma once
#include <cstdint>
#include "air_program.hpp"

namespace bpg {
namespace progdev {

// The register file.  A register numbered at run time cannot be a VGPR (the compiler would put the array in scratch), so
// the program's registers live in LDS as [reg][lane]: register r of lane l at word r * 256 + l (air_program.hip's header
// has the whole argument).  The value an instruction has just written also stays in a VGPR (`acc`).
extern __shared__ uint64_t lds_regs[];  // [n_regs][256]

struct LdsRegs {
  uint64_t* lane;  // register 0 of this lane
  uint64_t acc;    // the value of register `last`
  uint32_t last;   // wave-uniform
  __device__ __forceinline__ uint64_t get(uint32_t r) const { return r == last ? acc : lane[r * 256]; }
  __device__ __forceinline__ void set(uint32_t r, uint64_t v) {
    lane[r * 256] = v;
    acc = v;
    last = r;
  }
};
__device__ __forceinline__ LdsRegs lds_regs_of_lane() { return LdsRegs{lds_regs + threadIdx.x, 0, ~0u}; }

// beta_c^j, j < MAX_TUPLE, c < 2 (prog::beta_powers): a kernel argument, 2 KiB, read wave-uniformly
struct BetaTab {
  uint64_t v[2 * air::prog::MAX_TUPLE];
};

}  // namespace progdev
}  // namespace bpg
