// air_program.cpp -- the registry of run-time AIRs (air_program.hpp): the validator, the ids, the device images and the
// C ABI (include/bpg.h: bp_air_register, bp_air_unregister, bp_air_program_digest).
#include <cstring>
#include <map>
#include "air_program.hpp"
#include "common.hpp"
#include "mpt.hpp"

namespace bpg {
namespace air {
namespace prog {

namespace {

struct Registry {
  std::mutex mu;
  std::map<uint32_t, std::shared_ptr<const Program>> by_id;
};
// never destroyed: a program's device images must not be freed while the process tears the runtime down
Registry& registry() {
  static Registry* r = new Registry();
  return *r;
}

#define REFUSE(off, ...) return refuse((size_t)(off), __VA_ARGS__)
int refuse(size_t off, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int refuse(size_t off, const char* fmt, ...) {
  char msg[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(msg, sizeof(msg), fmt, ap);
  va_end(ap);
  return fail(BP_ERR_INVALID_INPUT, "bp_air_register: word %zu: %s", off, msg);
}

// Fills *p from the words or refuses them, naming the offending word.
int validate(const uint64_t* w, size_t n_words, Program* p) {
  if (!w || n_words < HDR_WORDS) REFUSE(0, "a program has at least the %u header words, got %zu", HDR_WORDS, n_words);
  if (w[0] != MAGIC && w[0] != MAGIC2 && w[0] != MAGIC3) REFUSE(0, "bad magic (expected \"BPGAIRP1\", \"BPGAIRP2\" or \"BPGAIRP3\")");
  const bool p3 = w[0] == MAGIC3, p2 = w[0] == MAGIC2 || p3;  // "BPGAIRP3" is "BPGAIRP2" with a kind in the port words
  const size_t hdr_words = p2 ? HDR_WORDS2 : HDR_WORDS;
  if (n_words < hdr_words)
    REFUSE(0, "a \"BPGAIRP%c\" program has at least the %u header words, got %zu", p3 ? '3' : '2', HDR_WORDS2, n_words);
  struct Range { uint32_t* out; uint64_t lo, hi; const char* name; };
  const Range hdr[9] = {{&p->n_cols, MIN_COLS, MAX_COLS, "n_cols"}, {&p->n_const, 0, MAX_CONST, "n_const"},
                        {&p->n_public, 0, MAX_PUBLIC, "n_public"}, {&p->degree, 1, MAX_DEGREE, "degree"},
                        {&p->n_constraints, 1, MAX_CONSTRAINTS, "n_constraints"}, {&p->n_families, 1, MAX_FAMILIES, "n_families"},
                        {&p->n_regs, 1, MAX_REGS, "n_regs"}, {&p->n_units, 1, MAX_UNITS, "n_units"}, {&p->n_code, 1, MAX_CODE, "n_code"}};
  for (uint32_t i = 0; i < 9; i++) {
    if (w[1 + i] < hdr[i].lo || w[1 + i] > hdr[i].hi)
      REFUSE(1 + i, "%s = %llu is outside %llu .. %llu", hdr[i].name, (unsigned long long)w[1 + i], (unsigned long long)hdr[i].lo,
             (unsigned long long)hdr[i].hi);
    *hdr[i].out = (uint32_t)w[1 + i];
  }
  if (p2) {
    if (w[10] > MAX_PORTS) REFUSE(10, "n_ports = %llu is outside 0 .. %u", (unsigned long long)w[10], MAX_PORTS);
    p->n_ports = (uint32_t)w[10];
    // bp_air_describe lists the program's families and then the ports': five per port where they fit, else three
    // interleaved ones for all ports, which always fit behind MAX_FAMILIES_WITH_PORTS of the program's own
    if (p->n_ports && p->n_families > MAX_FAMILIES_WITH_PORTS)
      REFUSE(6, "n_families = %u: a program with ports has at most %u families of its own (bp_air_describe lists the ports' behind them)",
             p->n_families, MAX_FAMILIES_WITH_PORTS);
  }
  const size_t fam0 = hdr_words, port0 = fam0 + 4 * (size_t)p->n_families, off0 = port0 + p->n_ports,
               code0 = off0 + p->n_units + p->n_ports + 1, total = code0 + p->n_code;
  const uint32_t n_all_units = p->n_units + p->n_ports;
  if (n_words != total) REFUSE(9, "the header's sizes make a program of %zu words, got %zu", total, n_words);
  p->off0 = off0;
  for (uint32_t l = 0; l < p->n_ports; l++) {
    uint64_t n_tuple = w[port0 + l];
    if (p3) {  // n_tuple | kind << 32
      const uint64_t kind = (w[port0 + l] >> 32) & 3;
      if (w[port0 + l] >> 34)
        REFUSE(port0 + l, "port %u: the port word 0x%llx has bits set above n_tuple | kind << 32", l, (unsigned long long)w[port0 + l]);
      if (kind >= PORT_KINDS) REFUSE(port0 + l, "port %u: kind %llu (0 product, 1 log with a bit filter, 2 log with a multiplicity)", l,
                                     (unsigned long long)kind);
      p->port_kind[l] = (uint32_t)kind;
      n_tuple &= 0xffffffffu;
    }
    if (n_tuple < 1 || n_tuple > MAX_TUPLE)
      REFUSE(port0 + l, "port %u: n_tuple = %llu is outside 1 .. %u", l, (unsigned long long)n_tuple, MAX_TUPLE);
    p->n_tuple[l] = (uint32_t)n_tuple;
  }
  // the family table tiles [0, n_constraints)
  std::vector<uint8_t> fam_of(p->n_constraints);
  uint64_t next = 0;
  for (uint32_t f = 0; f < p->n_families; f++) {
    const uint64_t* q = w + fam0 + 4 * (size_t)f;
    if (q[0] != next) REFUSE(fam0 + 4 * f, "family %u starts at constraint %llu, the families so far end at %llu: they must tile the list", f,
                             (unsigned long long)q[0], (unsigned long long)next);
    if (q[1] == 0 || q[1] > p->n_constraints - next)
      REFUSE(fam0 + 4 * f + 1, "family %u has %llu constraints, %llu are left of the list", f, (unsigned long long)q[1],
             (unsigned long long)(p->n_constraints - next));
    if (q[2] > 3) REFUSE(fam0 + 4 * f + 2, "family %u: kind %llu (0 all rows, 1 transition, 2 first row, 3 last row)", f, (unsigned long long)q[2]);
    if (q[3] == 0 || q[3] > p->degree)
      REFUSE(fam0 + 4 * f + 3, "family %u: degree %llu is outside 1 .. the program's degree %u", f, (unsigned long long)q[3], p->degree);
    // A first-row or last-row constraint is multiplied by a Lagrange polynomial of degree n - 1, not by a linear factor:
    // a family of degree d leaves a quotient of degree (d + 1)(n - 1) - n, which the 2^rate_bits n quotient
    // coefficients hold only for d <= 2^rate_bits (rate_bits 1 up to degree 3, else 3).  Above that an honest proof
    // fails the constraint check at zeta, so the program is refused here.
    if (q[2] >= 2 && q[3] > boundary_degree(p->degree))
      REFUSE(fam0 + 4 * f + 3, "family %u: a %s family of degree %llu; a program of degree %u takes them up to degree %u (the row's "
             "selector has degree n - 1)", f, q[2] == 2 ? "first-row" : "last-row", (unsigned long long)q[3], p->degree, boundary_degree(p->degree));
    p->families[f] = Family{(uint32_t)q[0], (uint32_t)q[1], (uint32_t)q[2], (uint32_t)q[3]};
    for (uint64_t i = 0; i < q[1]; i++) fam_of[next + i] = (uint8_t)f;
    next += q[1];
  }
  if (next != p->n_constraints)
    REFUSE(fam0 + 4 * (size_t)(p->n_families - 1) + 1, "the families cover %llu of the %u constraints: they must tile the list",
           (unsigned long long)next, p->n_constraints);
  // the unit table tiles the code
  if (w[off0] != 0) REFUSE(off0, "the first unit starts at code word %llu, not 0", (unsigned long long)w[off0]);
  for (uint32_t u = 0; u < n_all_units; u++)
    if (w[off0 + u + 1] <= w[off0 + u] || w[off0 + u + 1] > p->n_code)
      REFUSE(off0 + u + 1, "unit %u ends at code word %llu: units are non-empty, in order, inside the %u code words", u,
             (unsigned long long)w[off0 + u + 1], p->n_code);
  if (w[off0 + n_all_units] != p->n_code)
    REFUSE(off0 + n_all_units, "the last unit ends at code word %llu of %u", (unsigned long long)w[off0 + n_all_units], p->n_code);
  // the code, unit by unit: operands in range, registers written before they are read, degrees
  std::vector<uint8_t> emitted(p->n_constraints, 0);
  for (uint32_t u = 0; u < n_all_units; u++) {
    int deg[MAX_REGS];  // -1: not written in this unit
    for (uint32_t r = 0; r < MAX_REGS; r++) deg[r] = -1;
    // a port unit: the degree of every slot written so far (-1: never), slot 0 the filter
    const bool port_unit = u >= p->n_units;
    const uint32_t port = u - p->n_units;
    int slot_deg[MAX_TUPLE + 1];
    for (uint32_t j = 0; j <= MAX_TUPLE; j++) slot_deg[j] = -1;
    for (size_t pc = code0 + w[off0 + u], end = code0 + w[off0 + u + 1]; pc < end; pc++) {
      const uint64_t c = w[pc];
      const uint32_t op = (uint32_t)c & 0xff, d = (uint32_t)(c >> 8) & 0xff, a = (uint32_t)(c >> 16) & 0xffffff, b = (uint32_t)(c >> 40);
      if (op >= (p2 ? OP_COUNT2 : OP_COUNT)) REFUSE(pc, "unknown operation %u", op);
      if (op == OP_EMIT && port_unit) REFUSE(pc, "emit in port unit %u: a port's constraints are the library's", port);
      if (op == OP_PORT) {
        if (!port_unit) REFUSE(pc, "port in constraint unit %u: ports are fed by their own units", u);
        if (a != port) REFUSE(pc, "the unit of port %u feeds port %u", port, a);
        if (d > p->n_tuple[port]) REFUSE(pc, "slot %u of port %u, whose tuple has %u elements (slots 0 .. %u)", d, port, p->n_tuple[port], p->n_tuple[port]);
        if (b >= p->n_regs) REFUSE(pc, "register %u of %u", b, p->n_regs);
        if (deg[b] < 0) REFUSE(pc, "register %u is read before unit %u writes it", b, u);
        if (deg[b] > slot_deg[d]) slot_deg[d] = deg[b];
        continue;
      }
      if (op != OP_EMIT && d >= p->n_regs) REFUSE(pc, "destination register %u of %u", d, p->n_regs);
      auto reads = [&](uint32_t r) -> int {
        if (r >= p->n_regs) return refuse(pc, "register %u of %u", r, p->n_regs);
        if (deg[r] < 0) return refuse(pc, "register %u is read before unit %u writes it", r, u);
        return BP_OK;
      };
      switch (op) {
        case OP_LOC: case OP_NXT:
          if (a >= p->n_cols) REFUSE(pc, "column %u of %u", a, p->n_cols);
          deg[d] = 1;
          break;
        case OP_CST:
          if (a >= p->n_const) REFUSE(pc, "constant column %u of %u", a, p->n_const);
          deg[d] = 1;
          break;
        case OP_PUB:
          if (a >= p->n_public) REFUSE(pc, "public input %u of %u", a, p->n_public);
          deg[d] = 0;
          break;
        case OP_X: deg[d] = 1; break;
        case OP_IMM:
          if (pc + 1 >= end) REFUSE(pc, "imm without its constant word in unit %u", u);
          if (w[pc + 1] >= gl::P) REFUSE(pc + 1, "non-canonical immediate 0x%llx", (unsigned long long)w[pc + 1]);
          pc++;
          deg[d] = 0;
          break;
        case OP_ADD: case OP_SUB: case OP_MUL: {
          if (int rc = reads(a)) return rc;
          if (int rc = reads(b)) return rc;
          const int s = op == OP_MUL ? deg[a] + deg[b] : (deg[a] > deg[b] ? deg[a] : deg[b]);
          deg[d] = s > 255 ? 255 : s;  // (far past every family's bound already)
          break;
        }
        default: {  // OP_EMIT
          if (a >= p->n_constraints) REFUSE(pc, "constraint %u of %u", a, p->n_constraints);
          if (int rc = reads(b)) return rc;
          const Family& f = p->families[fam_of[a]];
          if (d != f.kind) REFUSE(pc, "emit of constraint %u carries kind %u, its family %u has kind %u", a, d, fam_of[a], f.kind);
          if ((uint32_t)deg[b] > f.degree)
            REFUSE(pc, "degree violation: constraint %u is emitted a value of degree %d, its family %u allows %u", a, deg[b], fam_of[a], f.degree);
          emitted[a] = 1;
        }
      }
    }
    if (port_unit) {
      int deg_t = 0;
      for (uint32_t j = 0; j <= p->n_tuple[port]; j++) {
        if (slot_deg[j] < 0) REFUSE(off0 + u, "port %u: slot %u (%s) is never written", port, j, j ? "a tuple element" : "the filter");
        if (j && slot_deg[j] > deg_t) deg_t = slot_deg[j];
      }
      const int deg_f = slot_deg[0];
      p->port_deg_f[port] = (uint32_t)deg_f;
      p->port_deg_t[port] = (uint32_t)deg_t;
      if (p->port_kind[port] != PORT_PRODUCT) {
        // a log port: (s - s') d - f on transitions, s d - f on the last row (d = gamma + v), f f - f for a bit filter
        const int deg_s = 1 + deg_t > deg_f ? 1 + deg_t : deg_f;
        if (deg_s > (int)p->degree)
          REFUSE(off0 + u, "degree violation: log port %u has a filter of degree %d and a tuple of degree %d, (s - s') d - f must fit the "
                 "program's degree %u", port, deg_f, deg_t, p->degree);
        if (deg_s > (int)boundary_degree(p->degree))
          REFUSE(off0 + u, "degree violation: log port %u has a filter of degree %d and a tuple of degree %d, the last-row constraint "
                 "s d - f takes degree %u in a program of degree %u", port, deg_f, deg_t, boundary_degree(p->degree), p->degree);
        if (p->port_kind[port] == PORT_LOG_BIT && 2 * deg_f > (int)p->degree)
          REFUSE(off0 + u, "degree violation: log port %u has a bit filter of degree %d, f f - f must fit the program's degree %u", port,
                 deg_f, p->degree);
        continue;
      }
      // f f - f on all rows, z - z' term on transitions, z - term on the last row (term = 1 + f (gamma + v - 1))
      if (2 * deg_f > (int)p->degree)
        REFUSE(off0 + u, "degree violation: port %u has a filter of degree %d, f f - f must fit the program's degree %u", port, deg_f, p->degree);
      if (1 + deg_f + deg_t > (int)p->degree)
        REFUSE(off0 + u, "degree violation: port %u has a filter of degree %d and a tuple of degree %d, z - z' term must fit the program's "
               "degree %u", port, deg_f, deg_t, p->degree);
      if (deg_f + deg_t > (int)boundary_degree(p->degree))
        REFUSE(off0 + u, "degree violation: port %u has a filter of degree %d and a tuple of degree %d, the last-row constraint z - term "
               "takes degree %u in a program of degree %u", port, deg_f, deg_t, boundary_degree(p->degree), p->degree);
    }
  }
  for (uint32_t i = 0; i < p->n_constraints; i++)
    if (!emitted[i]) REFUSE(fam0 + 4 * (size_t)fam_of[i], "constraint %u (family %u) is never emitted", i, fam_of[i]);
  p->words.assign(w, w + n_words);
  const mpt::H256 h = mpt::keccak256(reinterpret_cast<const uint8_t*>(w), n_words * 8);
  std::memcpy(p->digest, h.data(), 32);
  p->air_id = REGISTERED_BIT | (((uint32_t)h[0] | (uint32_t)h[1] << 8 | (uint32_t)h[2] << 16 | (uint32_t)h[3] << 24) & 0x7fffffffu);
  return BP_OK;
}

}  // namespace

Program::~Program() {
  for (auto& d : dev_images) (void)hipFree(d.second);
}

std::shared_ptr<const Program> find(uint32_t air_id) {
  if (!is_registered(air_id)) return nullptr;
  Registry& r = registry();
  std::lock_guard<std::mutex> lk(r.mu);
  auto it = r.by_id.find(air_id);
  return it == r.by_id.end() ? nullptr : it->second;
}

int device_image(const std::shared_ptr<const Program>& p, const uint64_t** d_image) {
  int dev = 0;
  BPG_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(p->dev_mu);
  for (auto& d : p->dev_images)
    if (d.first == dev) {
      *d_image = d.second;
      return BP_OK;
    }
  uint64_t* d = nullptr;
  const std::vector<uint64_t> image = p->image();
  BPG_HIP(hipMalloc(reinterpret_cast<void**>(&d), image.size() * 8));
  if (hipMemcpy(d, image.data(), image.size() * 8, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d);
    return fail(BP_ERR_DEVICE, "upload of AIR program 0x%08x failed", p->air_id);
  }
  p->dev_images.emplace_back(dev, d);
  *d_image = d;
  return BP_OK;
}

}  // namespace prog

uint32_t any_n_constraints(const Shape& s) {
  if (!prog::is_registered(s.air_id)) return n_constraints(s);
  const auto p = prog::find(s.air_id);
  return p ? p->n_constraints : 0;
}
uint32_t any_n_units(const Shape& s) {
  if (!prog::is_registered(s.air_id)) return n_units(s);
  const auto p = prog::find(s.air_id);
  return p ? p->n_units : 0;
}
uint32_t any_n_aux(const Shape& s) {
  if (!prog::is_registered(s.air_id)) return ctl::n_aux(s);
  const auto p = prog::find(s.air_id);
  return p ? p->n_aux() : 1;
}
uint32_t any_n_ctl_constraints(const Shape& s) {
  if (!prog::is_registered(s.air_id)) return ctl::n_constraints(s);
  const auto p = prog::find(s.air_id);
  return p ? p->n_ctl_constraints() : 2;
}

}  // namespace air
}  // namespace bpg

using namespace bpg;
namespace prog = bpg::air::prog;

extern "C" {

int bp_air_register(const uint64_t* program, size_t n_words, uint32_t* air_id_out) try {
  if (!air_id_out) return fail(BP_ERR_INVALID_INPUT, "bp_air_register: null air_id_out");
  auto p = std::make_shared<prog::Program>();
  if (int rc = prog::validate(program, n_words, p.get())) return rc;
  auto& r = prog::registry();
  std::lock_guard<std::mutex> lk(r.mu);
  auto it = r.by_id.find(p->air_id);
  if (it != r.by_id.end()) {
    if (it->second->words != p->words)
      return fail(BP_ERR_INVALID_INPUT, "bp_air_register: id 0x%08x is taken by another registered program (the ids are 31 bits of "
                  "Keccak-256): unregister that one first", p->air_id);
  } else {
    r.by_id.emplace(p->air_id, p);
  }
  *air_id_out = p->air_id;
  return BP_OK;
}
BPG_ABI_CATCH("bp_air_register")

int bp_air_unregister(uint32_t air_id) try {
  std::shared_ptr<const prog::Program> gone;  // (its device images are freed outside the lock, once nothing uses it)
  {
    auto& r = prog::registry();
    std::lock_guard<std::mutex> lk(r.mu);
    auto it = r.by_id.find(air_id);
    if (it == r.by_id.end()) return fail(BP_ERR_INVALID_INPUT, "bp_air_unregister: no program is registered as air_id 0x%08x", air_id);
    gone = it->second;
    r.by_id.erase(it);
  }
  return BP_OK;
}
BPG_ABI_CATCH("bp_air_unregister")

int bp_air_program_digest(uint32_t air_id, uint8_t out[32]) try {
  const auto p = prog::find(air_id);
  if (!p || !out) return fail(BP_ERR_INVALID_INPUT, "bp_air_program_digest: no program is registered as air_id 0x%08x, or null output", air_id);
  std::memcpy(out, p->digest, 32);
  return BP_OK;
}
BPG_ABI_CATCH("bp_air_program_digest")

}  // extern "C"
