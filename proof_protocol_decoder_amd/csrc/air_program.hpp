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
//
// "BPGAIRP2" is "BPGAIRP1" plus lookup PORTS (a filter and a tuple each: a side of a cross-table lookup, air.hpp section
// "cross-table lookups").  "BPGAIRP1" programs are untouched: their bytes, ids and digests do not move.
//   word 0        magic "BPGAIRP2"
//   1 .. 9        as above (n_units counts the constraint units only; n_regs covers both kinds of unit)
//   10            n_ports (0 .. 8)
//   then          the family table, as above
//   then          n_ports words: n_tuple of port l (1 .. 128)
//   then          n_units + n_ports + 1 code offsets: the constraint units, then port unit l = unit n_units + l
//   then          n_code code words, with one more operation
//   10 port dst = slot, a = port, b = register: slot 0 adds the register to the port's filter f, slot 1 + j to its
//                                 tuple element t_j (the partial sums add, in any order)
// Port units may load and compute but not emit; constraint units may not port; a port unit names its own port only.
// What follows from a port is the LIBRARY's, not the program's: with challenge set c = (beta_c, gamma_c),
// v_c = sum_j beta_c^j t_j and term_c = 1 + f (gamma_c + v_c - 1), a program with ports has 2 n_ports auxiliary columns
// (port l: z_{l,0}, z_{l,1} at 2l, 2l + 1, z_c[i] = prod_{i' >= i} term_c[i']) and 5 constraints per port after its own, at
// n_constraints + 5l: all rows f f - f; then for c = 0, 1 transition z_c - z_c' term_c, last row z_c - term_c (AIR 3's
// order).  Registration checks 2 deg f <= degree, 1 + deg f + max deg t_j <= degree and deg f + max deg t_j <=
// boundary_degree(degree) (z - term is a last-row constraint), that every slot 0 .. n_tuple is written and none beyond,
// and that a program with ports has at most 21 families of its own (bp_air_desc.families[24] holds them and the ports':
// five per port where they fit, else three interleaved ones).  A "BPGAIRP2" program with no port keeps the one
// constant product.
//
// "BPGAIRP3" is "BPGAIRP2" with a KIND per port: the port-table word of port l is n_tuple | kind << 32 (any other bit
// refused).  Kind 0 is the product port above.  Kinds 1 and 2 are LOG ports: the running column is a sum of fractions,
// s_c[i] = sum_{i' >= i} f[i'] / d_c[i'] with d_c = gamma_c + v_c, in the same two columns 2l, 2l + 1, and the same five
// constraint slots at n_constraints + 5l: slot 0, all rows, f f - f for kind 1 (the filter is a bit) and identically
// zero for kind 2 (the filter is a multiplicity: any field value); then for c = 0, 1 transition (s_c - s_c') d_c - f, last
// row s_c d_c - f.  Registration checks max(1 + deg t, deg f) <= degree and <= boundary_degree(degree), and for kind 1
// 2 deg f <= degree.  A link of log ports states, per tuple value, that the looking rows' filters sum to the looked
// rows'; membership of every sent tuple follows only when the looking filters are bits, which is why kind 1 exists and
// why f f - f is the library's.  Programs without a log port keep their "BPGAIRP1" / "BPGAIRP2" bytes, ids and proofs.
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
constexpr uint64_t MAGIC2 = 0x3250524941475042ULL;  // "BPGAIRP2"
constexpr uint64_t MAGIC3 = 0x3350524941475042ULL;  // "BPGAIRP3"
// a port's kind ("BPGAIRP3"): a running product; a running sum whose filter is a bit; ... is a multiplicity
constexpr uint32_t PORT_PRODUCT = 0, PORT_LOG_BIT = 1, PORT_LOG_MULT = 2, PORT_KINDS = 3;
constexpr uint32_t HDR_WORDS = 10, HDR_WORDS2 = 11;
constexpr uint32_t MAX_PORTS = 8, MAX_TUPLE = 128, PORT_CONSTRAINTS = 5, MAX_FAMILIES_WITH_PORTS = 21;
// The limits of a program (include/bpg.h states them).  MAX_REGS: the device keeps the registers in LDS, [reg][lane] for
// the 256 lanes of a workgroup = 2 KiB a register; 64 registers = 128 KiB of the CU's 160, so a registered program always
// fits.  n_cols / n_const: what check_cfg takes for any table.  degree: 9 is what rate_bits = 3 can divide out.
constexpr uint32_t MIN_COLS = 8, MAX_COLS = 65536, MAX_CONST = 4096, MAX_PUBLIC = 4, MAX_DEGREE = 9, MAX_CONSTRAINTS = 65536,
                   MAX_FAMILIES = 24, MAX_REGS = 64, MAX_UNITS = 256, MAX_CODE = 1u << 20;
constexpr uint32_t OP_LOC = 0, OP_NXT = 1, OP_CST = 2, OP_PUB = 3, OP_X = 4, OP_IMM = 5, OP_ADD = 6, OP_SUB = 7, OP_MUL = 8,
                   OP_EMIT = 9, OP_COUNT = 10, OP_PORT = 10, OP_COUNT2 = 11;
// the degree a first-row or last-row family may have in a program of `degree`: 2^rate_bits of the table's configuration
constexpr uint32_t boundary_degree(uint32_t degree) { return degree > 3 ? 8 : 2; }
constexpr uint32_t REGISTERED_BIT = 0x80000000u;
GL_HD bool is_registered(uint32_t air_id) { return (air_id & REGISTERED_BIT) != 0; }

// Code words [pc, end) of a program over the field policy T.  Regs: get(r) / set(r, v) -- an array on the host, LDS on
// the device.  Row: air.hpp's accessors.  Emit: air.hpp's consumer with one more method, emit(kind, index, value) =
// all / transition / first / last by the kind: ONE place in the loop feeds the consumer, so on the device the fold's
// accumulators (24 VGPRs) are updated at one point of the loop and stay where they are on every other path.  The words
// were validated at registration: nothing is checked here.
// Ports: the consumer of a port unit (PortAcc below), add(slot, value).  A constraint unit holds no port word, and a
// port unit no emit: each kind of unit runs the loop with the other's branch compiled out (PORT_UNIT), so the loop of
// a constraint unit is the one it was before ports existed.
template <class T, bool PORT_UNIT, class Regs, class Row, class Emit, class Ports>
GL_HD void run_unit(const uint64_t* code, uint32_t pc, uint32_t end, Regs& regs, const Row& row, Emit& out, Ports& ports) {
  typedef Ops<T> F;
#pragma unroll 1
  while (pc < end) {
    const uint64_t w = code[pc++];
    const uint32_t op = (uint32_t)w & 0xff, d = (uint32_t)(w >> 8) & 0xff, a = (uint32_t)(w >> 16) & 0xffffff, b = (uint32_t)(w >> 40);
    if constexpr (PORT_UNIT) {
      if (op == OP_PORT) {
        ports.add(d, regs.get(b));
        continue;
      }
    } else {
      if (op == OP_EMIT) {
        out.emit(d, a, regs.get(b));
        continue;
      }
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

struct NoPorts {
  template <class T>
  GL_HD void add(uint32_t, T) {}
};
template <class T, class Regs, class Row, class Emit>
GL_HD void run(const uint64_t* code, uint32_t pc, uint32_t end, Regs& regs, const Row& row, Emit& out) {
  NoPorts none;
  run_unit<T, false>(code, pc, end, regs, row, out, none);
}
struct NoEmit {
  template <class T>
  GL_HD void emit(uint32_t, uint32_t, T) {}
};
template <class T, class Regs, class Row, class Ports>
GL_HD void run_port(const uint64_t* code, uint32_t pc, uint32_t end, Regs& regs, const Row& row, Ports& ports) {
  NoEmit none;
  run_unit<T, true>(code, pc, end, regs, row, none, ports);
}

// What a port unit leaves: the filter and the tuple compressed by both challenge sets.  bpow: [2][MAX_TUPLE], beta_c^j
// (made once per proof; on the device the slot is wave-uniform, so the table is read as the code is).
template <class T>
struct PortAcc {
  const uint64_t* bpow;
  T f, v0, v1;
  GL_HD void reset() { f = v0 = v1 = Ops<T>::k(0); }
  GL_HD void add(uint32_t slot, T v) {
    typedef Ops<T> F;
    if (slot == 0) {
      f = F::add(f, v);
    } else {
      v0 = F::add(v0, F::mul(v, F::k(bpow[slot - 1])));
      v1 = F::add(v1, F::mul(v, F::k(bpow[MAX_TUPLE + slot - 1])));
    }
  }
  // term_c = 1 + f (gamma_c + v_c - 1)
  GL_HD T term(uint32_t c, const uint64_t ctl[4]) const {
    typedef Ops<T> F;
    return F::add(F::k(1), F::mul(f, F::sub(F::add(F::k(ctl[2 * c + 1]), c ? v1 : v0), F::k(1))));
  }
  // d_c = gamma_c + v_c: the denominator of a log port's fraction
  GL_HD T denom(uint32_t c, const uint64_t ctl[4]) const { return Ops<T>::add(Ops<T>::k(ctl[2 * c + 1]), c ? v1 : v0); }
};
inline void beta_powers(const uint64_t ctl[4], uint64_t out[2 * MAX_TUPLE]) {
  for (uint32_t c = 0; c < 2; c++) {
    uint64_t p = 1;
    for (uint32_t j = 0; j < MAX_TUPLE; j++, p = gl::mulc(p, ctl[2 * c])) out[c * MAX_TUPLE + j] = p;
  }
}
// The five constraints of port l, from what its unit left in `acc`: the caller of run hands them to the consumer the
// built-in tables' lookups go to (air::ctl::eval's order for AIR 3).  base: the index of the port's first constraint.
template <class T, class Row, class Emit>
GL_HD void port_constraints(uint32_t base, uint32_t l, const uint64_t ctl[4], const PortAcc<T>& acc, const Row& row, Emit& out) {
  typedef Ops<T> F;
  out.all(base, F::sub(F::mul(acc.f, acc.f), acc.f));
#pragma unroll 1
  for (uint32_t c = 0; c < 2; c++) {
    const T z = row.aux(2 * l + c), zn = row.aux_nxt(2 * l + c), term = acc.term(c, ctl);
    out.transition(base + 1 + 2 * c, F::sub(z, F::mul(zn, term)));
    out.last(base + 2 + 2 * c, F::sub(z, term));
  }
}

// The five slots of LOG port l (kind 1 or 2): slot 0 is f f - f for a bit filter and identically zero -- nothing is
// handed over -- for a multiplicity; s_c is the running sum in column 2l + c.
template <class T, class Row, class Emit>
GL_HD void log_port_constraints(uint32_t base, uint32_t l, uint32_t kind, const uint64_t ctl[4], const PortAcc<T>& acc, const Row& row,
                                Emit& out) {
  typedef Ops<T> F;
  if (kind == PORT_LOG_BIT) out.all(base, F::sub(F::mul(acc.f, acc.f), acc.f));
#pragma unroll 1
  for (uint32_t c = 0; c < 2; c++) {
    const T s = row.aux(2 * l + c), sn = row.aux_nxt(2 * l + c), d = acc.denom(c, ctl);
    out.transition(base + 1 + 2 * c, F::sub(F::mul(F::sub(s, sn), d), acc.f));
    out.last(base + 2 + 2 * c, F::sub(F::mul(s, d), acc.f));
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
  uint32_t n_ports = 0, n_tuple[MAX_PORTS] = {};  // "BPGAIRP2"
  uint32_t port_kind[MAX_PORTS] = {};             // "BPGAIRP3": PORT_PRODUCT / PORT_LOG_BIT / PORT_LOG_MULT
  uint32_t port_deg_f[MAX_PORTS] = {}, port_deg_t[MAX_PORTS] = {};  // the propagated degrees of a port's filter and tuple
  size_t off0 = 0;                                // where the unit offsets start in `words`
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
  const uint64_t* unit_off() const { return words.data() + off0; }  // n_units + n_ports + 1 of them
  const uint64_t* code() const { return unit_off() + n_units + n_ports + 1; }
  uint32_t deg_pow() const { return degree > 3 ? 3 : 1; }
  // a program without ports keeps the one constant running product AIR 4 and AIR 7 have
  uint32_t n_aux() const { return n_ports ? 2 * n_ports : 1; }
  uint32_t n_ctl_constraints() const { return n_ports ? PORT_CONSTRAINTS * n_ports : 2; }
  // bit l: port l is a log port (its two columns are running sums)
  uint32_t log_ports() const {
    uint32_t m = 0;
    for (uint32_t l = 0; l < n_ports; l++) m |= (uint32_t)(port_kind[l] != PORT_PRODUCT) << l;
    return m;
  }
  // The device image: the constraint units' offsets (n_units + 1), the code, then the port units' offsets
  // (n_ports + 1) -- behind the code, so the kernels that know nothing of ports read the image they always read -- and
  // behind those the ports' kinds (n_ports), which only the kernels of a program with a log port read.
  std::vector<uint64_t> image() const {
    std::vector<uint64_t> im(unit_off(), unit_off() + n_units + 1);
    im.insert(im.end(), code(), code() + n_code);
    im.insert(im.end(), unit_off() + n_units, unit_off() + n_units + n_ports + 1);
    im.insert(im.end(), port_kind, port_kind + n_ports);
    return im;
  }
  // unit u over the host field policy
  template <class T, class Row, class Emit>
  void eval_unit(uint32_t u, const Row& row, Emit& out) const {
    HostRegs<T> regs;
    run<T>(code(), (uint32_t)unit_off()[u], (uint32_t)unit_off()[u + 1], regs, row, out);
  }
  // port unit l into acc (reset here)
  template <class T, class Row>
  void eval_port(uint32_t l, const Row& row, PortAcc<T>& acc) const {
    HostRegs<T> regs;
    acc.reset();
    run_port<T>(code(), (uint32_t)unit_off()[n_units + l], (uint32_t)unit_off()[n_units + l + 1], regs, row, acc);
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
// the auxiliary columns and the lookup constraints: ctl::n_aux / ctl::n_constraints, or a registered program's ports'
uint32_t any_n_aux(const Shape& s);
uint32_t any_n_ctl_constraints(const Shape& s);

}  // namespace air
}  // namespace bpg
