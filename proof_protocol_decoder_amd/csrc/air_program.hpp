// air_program.hpp -- AIRs defined at run time: a table's constraints as a straight-line program of field operations,
// registered under an air_id of its own (bp_air_register) beside the built-in AIRs of air.hpp.
//
// The fourth instantiation of "one evaluation routine, several field policies": air.hpp's evaluators are C++ compiled
// three times (device K5, host verifier, trace checker); a program is DATA interpreted by ONE routine (run below) that is
// compiled the same three times -- over Ops<gl::Ext> at zeta (verifier.cpp), over Ops<gl::Ext> per constraint index
// (air_check.cpp) and over Ops<uint64_t> on the device (air_program.hip: K5 on the LDE coset, the checker on the trace
// domain) -- with air.hpp's row accessors and constraint consumers unchanged.
//
// The byte format (little-endian u64 words; include/bpg.h repeats it for callers):
//   word 0        magic "BPGAIRP1"
//   1 .. 9        n_cols, n_const, n_public, degree, n_constraints, n_families, n_regs, n_units, n_code
//   then          n_families x (first_index, count, kind, degree): the constraint list in bp_air_describe's shape; the
//                 families cover [0, n_constraints) in order, exactly once
//   then          n_units + 1 code offsets: unit u is code words [off[u], off[u + 1]), off[0] = 0, off[n_units] = n_code
//   then          n_code code words
// A code word is  op | dst << 8 | a << 16 | b << 40  (8 / 8 / 24 / 24 bits); registers do not live across units:
//   0 loc  dst, a = column        dst = trace column a at this row
//   1 nxt  dst, a = column        ... at the next row
//   2 cst  dst, a = column        preprocessed constant column a at this row
//   3 pub  dst, a = j             public input j
//   4 x    dst                    the evaluation point
//   5 imm  dst                    the NEXT code word, a canonical constant (< p)
//   6 add  dst, a, b              registers a + b          7 sub: a - b          8 mul: a * b
//   9 emit dst = kind, a = constraint index, b = register: adds the register to constraint a; the kind repeats the
//                                 family's (checked at registration), so the interpreter looks nothing up
// An index may be emitted several times (the partial sums add) and in any order, as with the built-in units.
#pragma once
#include <cstdint>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>
#include "air.hpp"

namespace bpg {
namespace air {
namespace prog {

constexpr uint64_t MAGIC = 0x3150524941475042ULL;  // "BPGAIRP1"
constexpr uint32_t HDR_WORDS = 10;
// The limits of a program (include/bpg.h states them).  MAX_REGS: the device keeps the registers in LDS, [reg][lane] for
// the 256 lanes of a workgroup = 2 KiB a register; 64 registers = 128 KiB of the CU's 160, so a registered program always
// fits.  n_cols / n_const: what check_cfg takes for any table.  degree: 9 is what rate_bits = 3 can divide out.
constexpr uint32_t MIN_COLS = 8, MAX_COLS = 65536, MAX_CONST = 4096, MAX_PUBLIC = 4, MAX_DEGREE = 9, MAX_CONSTRAINTS = 65536,
                   MAX_FAMILIES = 24, MAX_REGS = 64, MAX_UNITS = 256, MAX_CODE = 1u << 20;
constexpr uint32_t OP_LOC = 0, OP_NXT = 1, OP_CST = 2, OP_PUB = 3, OP_X = 4, OP_IMM = 5, OP_ADD = 6, OP_SUB = 7, OP_MUL = 8,
                   OP_EMIT = 9, OP_COUNT = 10;
// the degree a first-row or last-row family may have in a program of `degree`: 2^rate_bits of the table's configuration
constexpr uint32_t boundary_degree(uint32_t degree) { return degree > 3 ? 8 : 2; }
constexpr uint32_t REGISTERED_BIT = 0x80000000u;
GL_HD bool is_registered(uint32_t air_id) { return (air_id & REGISTERED_BIT) != 0; }

// Code words [pc, end) of a program over the field policy T.  Regs: get(r) / set(r, v) -- an array on the host, LDS on
// the device.  Row: air.hpp's accessors.  Emit: air.hpp's consumer with one more method, emit(kind, index, value) =
// all / transition / first / last by the kind: ONE place in the loop feeds the consumer, so on the device the fold's
// accumulators (24 VGPRs) are updated at one point of the loop and stay where they are on every other path.  The words
// were validated at registration: nothing is checked here.
template <class T, class Regs, class Row, class Emit>
GL_HD void run(const uint64_t* code, uint32_t pc, uint32_t end, Regs& regs, const Row& row, Emit& out) {
  typedef Ops<T> F;
#pragma unroll 1
  while (pc < end) {
    const uint64_t w = code[pc++];
    const uint32_t op = (uint32_t)w & 0xff, d = (uint32_t)(w >> 8) & 0xff, a = (uint32_t)(w >> 16) & 0xffffff, b = (uint32_t)(w >> 40);
    if (op == OP_EMIT) {
      out.emit(d, a, regs.get(b));
      continue;
    }
    T v;
    switch (op) {
      case OP_LOC: v = row.loc(a); break;
      case OP_NXT: v = row.nxt(a); break;
      case OP_CST: v = row.cst(a); break;
      case OP_PUB: v = F::k(row.pub(a)); break;
      case OP_X: v = row.x(); break;
      case OP_IMM: v = F::k(code[pc++]); break;
      case OP_ADD: v = F::add(regs.get(a), regs.get(b)); break;
      case OP_SUB: v = F::sub(regs.get(a), regs.get(b)); break;
      default: v = F::mul(regs.get(a), regs.get(b)); break;  // OP_MUL
    }
    regs.set(d, v);
  }
}

template <class T>
struct HostRegs {
  T r[MAX_REGS];
  T get(uint32_t i) const { return r[i]; }
  void set(uint32_t i, T v) { r[i] = v; }
};

struct Family {
  uint32_t first_index, count, kind, degree;
};
// A validated program.  `words` are the registered bytes (what the id and the digest are taken from).
struct Program {
  uint32_t air_id = 0;
  uint32_t n_cols = 0, n_const = 0, n_public = 0, degree = 0, n_constraints = 0, n_families = 0, n_regs = 0, n_units = 0, n_code = 0;
  Family families[MAX_FAMILIES] = {};
  std::vector<uint64_t> words;
  uint8_t digest[32] = {};
  // the image on every device that has used the program (device_image); freed with the program
  mutable std::mutex dev_mu;
  mutable std::vector<std::pair<int, uint64_t*>> dev_images;
  Program() = default;
  Program(const Program&) = delete;
  Program& operator=(const Program&) = delete;
  ~Program();
  const uint64_t* unit_off() const { return words.data() + HDR_WORDS + 4 * (size_t)n_families; }
  const uint64_t* code() const { return unit_off() + n_units + 1; }
  uint32_t deg_pow() const { return degree > 3 ? 3 : 1; }
  // the device image: unit offsets, then code (n_units + 1 + n_code words)
  const uint64_t* image() const { return unit_off(); }
  size_t image_words() const { return (size_t)n_units + 1 + n_code; }
  // unit u over the host field policy
  template <class T, class Row, class Emit>
  void eval_unit(uint32_t u, const Row& row, Emit& out) const {
    HostRegs<T> regs;
    run<T>(code(), (uint32_t)unit_off()[u], (uint32_t)unit_off()[u + 1], regs, row, out);
  }
};

// air_program.cpp: the registry.  A handle keeps its program alive across bp_air_unregister.
std::shared_ptr<const Program> find(uint32_t air_id);
// the program's image on the CURRENT device: uploaded at its first use there, kept until the program is unregistered
int device_image(const std::shared_ptr<const Program>& p, const uint64_t** d_image);

}  // namespace prog

// the AIR's own constraints / units of a built-in or a registered id (0 for a registered id nobody registered:
// check_cfg has refused it before anything asks)
uint32_t any_n_constraints(const Shape& s);
uint32_t any_n_units(const Shape& s);

}  // namespace air
}  // namespace bpg
