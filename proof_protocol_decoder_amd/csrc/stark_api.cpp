// stark_api.cpp -- C ABI entry for one synthetic-AIR table proof (include/bpg.h, L0.5).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <random>
#include <string>
#include <vector>
#include "prover.hpp"
#include "set_check.hpp"

using namespace bpg;

namespace {
constexpr uint32_t LONE_PI_LEN = 4;
void lone_public_input_list(uint64_t seed, uint64_t out[LONE_PI_LEN]) {
  for (uint64_t j = 0; j < LONE_PI_LEN; j++) {
    uint64_t z = (seed ^ ((0x50 + j) << 32)) + 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    out[j] = gl::canon(z ^ (z >> 31));
  }
}
}  // namespace
namespace {
// One parked worker (stream + arena) per device: a 2^20 x 2432 table needs a ~100 GB arena, and
// hipFree + hipMalloc of that much costs seconds -- several times the proof itself.  A call takes
// the parked worker if its arena is large enough (concurrent calls simply make their own), and parks
// its worker again when the slot is free.  bp_release_cached_memory() empties the slots.
std::mutex g_park_mu;
std::vector<Worker*> g_parked;  // index = device

void park_worker(Worker* w);

Worker* take_worker(int device, size_t bytes, int* rc) {
  Worker* w = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_park_mu);
    if (device >= 0 && (size_t)device < g_parked.size() && g_parked[device]) {
      w = g_parked[device];
      g_parked[device] = nullptr;
    }
  }
  if (w && w->arena.capacity() >= bytes) {
    if (hipSetDevice(device) != hipSuccess) {
      *rc = fail(BP_ERR_DEVICE, "hipSetDevice(%d) failed", device);
      park_worker(w);
      return nullptr;
    }
    w->arena.release(0);
    w->abort_flag = nullptr;
    *rc = BP_OK;
    return w;
  }
  if (w) {
    w->destroy();
    delete w;
  }
  w = new Worker();
  *rc = w->init(device, bytes);
  if (*rc) {
    w->destroy();
    delete w;
    return nullptr;
  }
  return w;
}
void park_worker(Worker* w) {
  {
    std::lock_guard<std::mutex> lk(g_park_mu);
    if (w->device >= 0) {
      if (g_parked.size() <= (size_t)w->device) g_parked.resize(w->device + 1, nullptr);
      if (!g_parked[w->device]) {
        g_parked[w->device] = w;
        return;
      }
    }
  }
  w->destroy();
  delete w;
}
}  // namespace

// ---- table sets: several caller traces linked port to port, proven on one transcript (include/bpg.h) ---------

namespace {
constexpr uint64_t SET_MAGIC = 0x3154455354475042ULL;  // "BPGTSET1"
constexpr uint32_t SET_MAX_TABLES = 8, SET_MAX_LINKS = 16, SET_MAX_LOOKING = 8;

// the lookup ports of a member: a registered program's own, a built-in's product columns in air::DESC order
// (port l = columns first_product + 2l + c); 0: the id is no side of any lookup
uint32_t set_ports_of(uint32_t air_id, uint32_t* first_product) {
  *first_product = 0;
  if (const auto p = air::prog::find(air_id)) return p->n_ports;
  const air::Desc* d = air::info(air_id);
  if (!d || !d->in_pair) return 0;
  *first_product = d->first_product;
  return (d->n_aux - d->first_product) / 2;
}
struct SetShape {
  StarkCfg cfg[SET_MAX_TABLES];
  uint32_t n_ports[SET_MAX_TABLES], first_product[SET_MAX_TABLES];
  uint32_t log_ports[SET_MAX_TABLES];  // bit l: port l of the table is a log port (a registered "BPGAIRP3" program's)
  bool log_link[SET_MAX_LINKS];        // the link's ports are log ports: its identity is a sum
};
// the statement of a set, refused or accepted without touching a device
int check_set(const char* who, const bp_set_table* tables, uint32_t n_tables, const bp_set_link* links, uint32_t n_links, SetShape* out) {
  if (!tables || !links) return fail(BP_ERR_INVALID_INPUT, "%s: null argument", who);
  if (n_tables < 1 || n_tables > SET_MAX_TABLES) return fail(BP_ERR_INVALID_INPUT, "%s: a set has 1 .. %u tables, got %u", who, SET_MAX_TABLES, n_tables);
  if (n_links < 1 || n_links > SET_MAX_LINKS) return fail(BP_ERR_INVALID_INPUT, "%s: a set has 1 .. %u links, got %u", who, SET_MAX_LINKS, n_links);
  uint32_t used[SET_MAX_TABLES][16] = {};
  for (uint32_t t = 0; t < n_tables; t++) {
    const bp_stark_cfg& c = tables[t].cfg;
    out->cfg[t] = StarkCfg{c.log_n, c.n_cols, c.n_const, c.deg_pow, c.rate_bits, c.cap_height, c.num_queries, c.pow_bits, c.arity_bits,
                           c.final_poly_bits, tables[t].air_id};
    if (int rc = check_cfg(out->cfg[t])) {
      const std::string why = bp_last_error();
      return fail(rc, "%s: table %u: %s", who, t, why.c_str());
    }
    out->n_ports[t] = set_ports_of(tables[t].air_id, &out->first_product[t]);
    const auto program = air::prog::find(tables[t].air_id);
    out->log_ports[t] = program ? program->log_ports() : 0;  // a built-in member's ports are product ports
    if (!out->n_ports[t])
      return fail(BP_ERR_INVALID_INPUT, "%s: table %u: air_id %u (0x%08x) has no lookup port: a member is a registered program with ports or "
                  "one of the built-in AIRs 1, 2, 3, 5, 6", who, t, tables[t].air_id, tables[t].air_id);
    if (tables[t].pub)
      for (int j = 0; j < 4; j++)
        if (tables[t].pub[j] >= gl::P) return fail(BP_ERR_INVALID_INPUT, "%s: table %u: non-canonical public input", who, t);
    if (!tables[t].pub && (tables[t].air_id == air::PLONK || (program && program->n_public)))
      return fail(BP_ERR_INVALID_INPUT, "%s: table %u: the AIR reads public inputs: pass four words", who, t);
  }
  for (uint32_t k = 0; k < n_links; k++) {
    const bp_set_link& l = links[k];
    if (l.n_looking < 1 || l.n_looking > SET_MAX_LOOKING)
      return fail(BP_ERR_INVALID_INPUT, "%s: link %u has %u looking ports (1 .. %u)", who, k, l.n_looking, SET_MAX_LOOKING);
    for (uint32_t m = 0; m <= l.n_looking; m++) {
      const bp_set_port& e = m < l.n_looking ? l.looking[m] : l.looked;
      if (e.table >= n_tables) return fail(BP_ERR_INVALID_INPUT, "%s: link %u names table %u of %u", who, k, e.table, n_tables);
      if (e.port >= out->n_ports[e.table])
        return fail(BP_ERR_INVALID_INPUT, "%s: link %u names port %u of table %u, which has %u", who, k, e.port, e.table, out->n_ports[e.table]);
      if (used[e.table][e.port]++)
        return fail(BP_ERR_INVALID_INPUT, "%s: port %u of table %u is named twice (link %u): a port is in exactly one link", who, e.port, e.table, k);
      // product ports multiply, log ports add: one link takes one kind.  (Both ends may be in the same table: a table
      // that range-checks itself.)
      const bool is_log = (out->log_ports[e.table] >> e.port) & 1;
      if (m == 0) out->log_link[k] = is_log;
      else if (is_log != out->log_link[k])
        return fail(BP_ERR_INVALID_INPUT, "%s: link %u mixes product and log ports: port %u of table %u is a %s port, port %u of table %u a "
                    "%s port", who, k, e.port, e.table, is_log ? "log" : "product", l.looking[0].port, l.looking[0].table,
                    is_log ? "product" : "log");
    }
  }
  for (uint32_t t = 0; t < n_tables; t++)
    for (uint32_t l = 0; l < out->n_ports[t]; l++)
      if (!used[t][l])
        return fail(BP_ERR_INVALID_INPUT, "%s: port %u of table %u is in no link: an unlinked port proves nothing about the other tables (prove "
                    "the table alone with bp_stark_prove_trace)", who, l, t);
  return BP_OK;
}
// the statement, as both sides observe it before any commitment
int observe_set(Challenger& ch, const bp_set_table* tables, uint32_t n_tables, const bp_set_link* links, uint32_t n_links, const SetShape& sh) {
  ch.observe(SET_MAGIC % gl::P);
  ch.observe(n_tables);
  ch.observe(n_links);
  for (uint32_t t = 0; t < n_tables; t++) {
    const StarkCfg& c = sh.cfg[t];
    const uint64_t w[5] = {c.air_id, c.log_n, c.n_cols, c.n_const, c.rate_bits};
    ch.observe(w, 5);
    if (air::prog::is_registered(c.air_id)) {  // the whole digest: a verifier does not trust 31 bits of id
      const auto p = air::prog::find(c.air_id);
      if (!p) return fail(BP_ERR_INVALID_INPUT, "AIR program 0x%08x was unregistered", c.air_id);
      for (int j = 0; j < 8; j++) {
        uint32_t d;
        std::memcpy(&d, p->digest + 4 * j, 4);
        ch.observe(d);
      }
    }
  }
  for (uint32_t k = 0; k < n_links; k++) {
    ch.observe(links[k].n_looking);
    for (uint32_t m = 0; m <= links[k].n_looking; m++) {
      const bp_set_port& e = m < links[k].n_looking ? links[k].looking[m] : links[k].looked;
      ch.observe(e.table);
      ch.observe(e.port);
    }
  }
  return BP_OK;
}
// Every link on the first-row openings: for both challenge sets the product of the looking ports' values is the looked
// port's (check_lookups' identity, txn_tables.cpp, with a looking count); for a link of log ports, their sum.
int check_links(const SetShape& sh, const bp_set_link* links, uint32_t n_links, const std::vector<uint64_t>* proof) {
  for (uint32_t k = 0; k < n_links; k++) {
    const bp_set_link& l = links[k];
    for (uint32_t c = 0; c < 2; c++) {
      auto first_row = [&](const bp_set_port& e) {
        const ProofLayout L = proof_layout(sh.cfg[e.table]);
        const uint64_t* v = proof[e.table].data() + L.open_first + 2 * (size_t)(sh.first_product[e.table] + 2 * e.port + c);
        return gl::Ext{v[0], v[1]};
      };
      gl::Ext a = gl::ext(sh.log_link[k] ? 0 : 1);
      for (uint32_t m = 0; m < l.n_looking; m++) a = sh.log_link[k] ? gl::add(a, first_row(l.looking[m])) : gl::mul(a, first_row(l.looking[m]));
      const gl::Ext b = first_row(l.looked);
      if (a.c0 != b.c0 || a.c1 != b.c1)
        return fail(BP_ERR_VERIFY, "link %u does not hold (challenge set %u): port %u of table %u%s asks for tuples that port %u of table %u "
                    "does not expose", k, c, l.looking[0].port, l.looking[0].table, l.n_looking > 1 ? " (and the link's other looking ports)" : "",
                    l.looked.port, l.looked.table);
    }
  }
  return BP_OK;
}
size_t table_arena_bytes(const StarkCfg& c, bool packed) {
  const uint64_t N = (uint64_t)1 << c.log_n, M = N << c.rate_bits;
  const size_t cols = (size_t)c.n_cols + c.n_const + c.n_cols / 8 + (2u << c.rate_bits) + 64;
  return cols * (2 * N + M) * 8 + (size_t)80 * M * 8 + ((size_t)c.n_cols / 32 + 64) * 8 * N * 8 + (packed ? (size_t)c.n_cols * N * 8 : 0);
}
}  // namespace

extern "C" {

int bp_stark_prove_table_set(const bp_set_table* tables, uint32_t n_tables, const bp_set_link* links, uint32_t n_links, uint32_t flags,
                             int device, uint8_t** out, size_t* out_len) try {
  if (!out || !out_len) return fail(BP_ERR_INVALID_INPUT, "bp_stark_prove_table_set: null argument");
  if (flags & ~(uint32_t)BP_SET_SKIP_LINK_CHECK) return fail(BP_ERR_INVALID_INPUT, "bp_stark_prove_table_set: unknown flags 0x%x", flags);
  SetShape sh;
  int rc = check_set("bp_stark_prove_table_set", tables, n_tables, links, n_links, &sh);
  if (rc) return rc;
  size_t bytes = 64u << 20;
  for (uint32_t t = 0; t < n_tables; t++) {
    const uint64_t N = (uint64_t)1 << sh.cfg[t].log_n;
    if (!tables[t].d_trace || (sh.cfg[t].n_const && !tables[t].d_consts))
      return fail(BP_ERR_INVALID_INPUT, "bp_stark_prove_table_set: table %u: null trace, or the AIR reads %u constant columns and none are given", t,
                  sh.cfg[t].n_const);
    if (tables[t].stride < N)
      return fail(BP_ERR_INVALID_INPUT, "bp_stark_prove_table_set: table %u: column stride %llu is shorter than the %llu-row trace", t,
                  (unsigned long long)tables[t].stride, (unsigned long long)N);
    bytes += table_arena_bytes(sh.cfg[t], tables[t].stride != N);
  }
  Worker* wp = take_worker(device, bytes, &rc);
  if (!wp) return rc;
  Worker& w = *wp;
  struct Parker {
    Worker* w;
    ~Parker() { park_worker(w); }
  } parker{wp};
  auto body = [&]() -> int {
    Challenger ch;
    int r2 = observe_set(ch, tables, n_tables, links, n_links, sh);
    if (r2) return r2;
    // every commitment before the lookup challenges exist: per table the constants (if any), the trace, the public inputs
    Committed consts[SET_MAX_TABLES], trace[SET_MAX_TABLES];
    const uint64_t* d_tv[SET_MAX_TABLES];
    Ctl ctl[SET_MAX_TABLES];
    for (uint32_t t = 0; t < n_tables; t++) {
      const StarkCfg& c = sh.cfg[t];
      const uint64_t N = (uint64_t)1 << c.log_n;
      if (c.n_const) {
        if ((r2 = commit(w, tables[t].d_consts, c.n_const, c.log_n, c.rate_bits, c.cap_height, false, &consts[t]))) return r2;
        ch.observe(consts[t].cap.data(), consts[t].cap.size());
      }
      d_tv[t] = tables[t].d_trace;
      if (tables[t].stride != N) {
        uint64_t* packed = w.arena.alloc_words((size_t)c.n_cols * N);
        if (!packed) return fail(BP_ERR_DEVICE, "arena exhausted");
        BPG_HIP(hipMemcpy2DAsync(packed, N * 8, tables[t].d_trace, tables[t].stride * 8, N * 8, c.n_cols, hipMemcpyDeviceToDevice, w.stream));
        d_tv[t] = packed;
      }
      if ((r2 = commit(w, d_tv[t], c.n_cols, c.log_n, c.rate_bits, c.cap_height, false, &trace[t]))) return r2;
      ch.observe(trace[t].cap.data(), trace[t].cap.size());
      if (tables[t].pub)
        for (int j = 0; j < 4; j++) ctl[t].pub[j] = tables[t].pub[j];
      ch.observe(ctl[t].pub, 4);
    }
    uint64_t v[4];
    for (int i = 0; i < 4; i++) v[i] = ch.challenge();
    // the table proofs in order, one transcript threaded through all of them (prove_tables, proofgen.cpp)
    std::vector<uint64_t> proof[SET_MAX_TABLES];
    for (uint32_t t = 0; t < n_tables; t++) {
      for (int i = 0; i < 4; i++) ctl[t].v[i] = v[i];
      const size_t mark = w.arena.mark();
      if ((r2 = stark_prove(w, sh.cfg[t], sh.cfg[t].n_const ? &consts[t] : nullptr, trace[t], d_tv[t], ctl[t], ch, proof[t]))) return r2;
      w.arena.release(mark);
    }
    if (!(flags & BP_SET_SKIP_LINK_CHECK))
      if ((r2 = check_links(sh, links, n_links, proof))) return r2;
    std::vector<uint64_t> blob = {SET_MAGIC, n_tables, n_links, v[0], v[1], v[2], v[3]};
    for (uint32_t k = 0; k < n_links; k++) {
      blob.push_back(links[k].n_looking);
      for (uint32_t m = 0; m <= links[k].n_looking; m++) {
        const bp_set_port& e = m < links[k].n_looking ? links[k].looking[m] : links[k].looked;
        blob.push_back(e.table);
        blob.push_back(e.port);
      }
    }
    for (uint32_t t = 0; t < n_tables; t++) {
      const uint64_t hdr[4] = {sh.cfg[t].air_id, sh.cfg[t].log_n, sh.cfg[t].n_cols, proof[t].size()};
      blob.insert(blob.end(), hdr, hdr + 4);
      blob.insert(blob.end(), proof[t].begin(), proof[t].end());
    }
    *out_len = blob.size() * 8;
    *out = static_cast<uint8_t*>(std::malloc(*out_len));
    if (!*out) return fail(BP_ERR_DEVICE, "host allocation failed");
    std::memcpy(*out, blob.data(), *out_len);
    return BP_OK;
  };
  rc = body();
  if (rc) {
    const std::string why = bp_last_error();  // (the wait below must not lose the message)
    (void)hipStreamSynchronize(w.stream);
    return fail(rc, "%s", why.c_str());
  }
  if ((rc = w.wait())) {  // the caller gets no buffer with a failure
    std::free(*out);
    *out = nullptr;
    *out_len = 0;
  }
  return rc;
}
BPG_ABI_CATCH("bp_stark_prove_table_set")

// The statement is the VERIFIER's: tables (device pointers ignored), constants caps and links are the caller's own; the
// container only supplies the proofs.  Host only.
int bp_stark_verify_table_set(const bp_set_table* tables, uint32_t n_tables, const uint64_t* const* const_caps, const bp_set_link* links,
                              uint32_t n_links, const uint8_t* bytes, size_t len) try {
  if (!bytes) return fail(BP_ERR_INVALID_INPUT, "bp_stark_verify_table_set: null argument");
  SetShape sh;
  int rc = check_set("bp_stark_verify_table_set", tables, n_tables, links, n_links, &sh);
  if (rc) return rc;
  for (uint32_t t = 0; t < n_tables; t++)
    if (sh.cfg[t].n_const && !(const_caps && const_caps[t]))
      return fail(BP_ERR_INVALID_INPUT, "bp_stark_verify_table_set: table %u has constant columns: pass their cap", t);
  if (len % 8 || len < 7 * 8) return fail(BP_ERR_VERIFY, "table set: truncated");
  const size_t n_words = len / 8;
  std::vector<uint64_t> Wv(n_words);
  std::memcpy(Wv.data(), bytes, len);
  const uint64_t* W = Wv.data();
  if (W[0] != SET_MAGIC) return fail(BP_ERR_VERIFY, "table set: bad magic (expected \"BPGTSET1\")");
  if (W[1] != n_tables || W[2] != n_links)
    return fail(BP_ERR_VERIFY, "table set: the container holds %llu tables and %llu links, the statement %u and %u", (unsigned long long)W[1],
                (unsigned long long)W[2], n_tables, n_links);
  size_t off = 7;
  for (uint32_t k = 0; k < n_links; k++) {
    const bp_set_link& l = links[k];
    if (off + 3 + 2 * (size_t)l.n_looking > n_words) return fail(BP_ERR_VERIFY, "table set: truncated at link %u", k);
    bool same = W[off] == l.n_looking;
    for (uint32_t m = 0; same && m <= l.n_looking; m++) {
      const bp_set_port& e = m < l.n_looking ? l.looking[m] : l.looked;
      same = W[off + 1 + 2 * m] == e.table && W[off + 2 + 2 * m] == e.port;
    }
    if (!same) return fail(BP_ERR_VERIFY, "table set: link %u of the container is not link %u of the statement", k, k);
    off += 3 + 2 * (size_t)l.n_looking;
  }
  std::vector<uint64_t> proof[SET_MAX_TABLES];
  ProofLayout L[SET_MAX_TABLES];
  for (uint32_t t = 0; t < n_tables; t++) {
    const StarkCfg& c = sh.cfg[t];
    L[t] = proof_layout(c);
    if (off + 4 > n_words) return fail(BP_ERR_VERIFY, "table set: truncated at table %u", t);
    if (W[off] != c.air_id || W[off + 1] != c.log_n || W[off + 2] != c.n_cols || W[off + 3] != L[t].total)
      return fail(BP_ERR_VERIFY, "table set: table %u is proven as air_id 0x%llx, 2^%llu rows x %llu columns in %llu words; the statement is "
                  "0x%x, 2^%u x %u in %zu", t, (unsigned long long)W[off], (unsigned long long)W[off + 1], (unsigned long long)W[off + 2],
                  (unsigned long long)W[off + 3], c.air_id, c.log_n, c.n_cols, L[t].total);
    off += 4;
    if (off + L[t].total > n_words) return fail(BP_ERR_VERIFY, "table set: truncated in table %u", t);
    proof[t].assign(W + off, W + off + L[t].total);
    off += L[t].total;
    // the header words stark_verify does not look at: the container must be exactly what the prover wrote
    const uint64_t* P = proof[t].data();
    if (P[4] != L[t].n_aux || P[5] != L[t].n_quot || P[7] != c.cap_height || P[11] != c.deg_pow || P[12] != c.pow_bits || P[13] != c.arity_bits || P[15] != 0)
      return fail(BP_ERR_VERIFY, "table set: table %u: proof header does not match the statement", t);
  }
  if (off != n_words) return fail(BP_ERR_VERIFY, "table set: trailing words");
  Challenger ch;
  if ((rc = observe_set(ch, tables, n_tables, links, n_links, sh))) return rc;
  Ctl ctl[SET_MAX_TABLES];
  for (uint32_t t = 0; t < n_tables; t++) {
    if (sh.cfg[t].n_const) ch.observe(const_caps[t], L[t].cap_words);
    ch.observe(proof[t].data() + L[t].trace_cap, L[t].cap_words);
    if (tables[t].pub)
      for (int j = 0; j < 4; j++) ctl[t].pub[j] = tables[t].pub[j];
    ch.observe(ctl[t].pub, 4);
  }
  for (int i = 0; i < 4; i++) {
    const uint64_t v = ch.challenge();
    if (v != W[3 + i]) return fail(BP_ERR_VERIFY, "table set: the lookup challenges do not follow from the statement and the commitments");
    for (uint32_t t = 0; t < n_tables; t++) ctl[t].v[i] = v;
  }
  for (uint32_t t = 0; t < n_tables; t++)
    if ((rc = stark_verify(sh.cfg[t], sh.cfg[t].n_const ? const_caps[t] : nullptr, ctl[t], ch, proof[t].data(), proof[t].size()))) {
      const std::string why = bp_last_error();
      return fail(rc, "table set: table %u: %s", t, why.c_str());
    }
  return check_links(sh, links, n_links, proof);
}
BPG_ABI_CATCH("bp_stark_verify_table_set")

// The pre-flight of a set (include/bpg.h): every member's own constraints through bp_air_check_trace, every link's
// balance on the device (set_check.hip).  Nothing is committed or proven; every table and every link is reported.
int bp_check_table_set(const bp_set_table* tables, uint32_t n_tables, const bp_set_link* links, uint32_t n_links, int device,
                       bp_set_report* out) try {
  if (!out) return fail(BP_ERR_INVALID_INPUT, "bp_check_table_set: null argument");
  SetShape sh;
  int rc = check_set("bp_check_table_set", tables, n_tables, links, n_links, &sh);
  if (rc) return rc;
  for (uint32_t t = 0; t < n_tables; t++) {
    const uint64_t N = (uint64_t)1 << sh.cfg[t].log_n;
    if (!tables[t].d_trace || (sh.cfg[t].n_const && !tables[t].d_consts))
      return fail(BP_ERR_INVALID_INPUT, "bp_check_table_set: table %u: null trace, or the AIR reads %u constant columns and none are given", t,
                  sh.cfg[t].n_const);
    if (tables[t].stride < N)
      return fail(BP_ERR_INVALID_INPUT, "bp_check_table_set: table %u: column stride %llu is shorter than the %llu-row trace", t,
                  (unsigned long long)tables[t].stride, (unsigned long long)N);
  }
  std::memset(out, 0, sizeof(*out));
  int before = 0;
  BPG_HIP(hipGetDevice(&before));
  BPG_HIP(hipSetDevice(device));
  struct Back { int d; ~Back() { (void)hipSetDevice(d); } } back{before};
  hipStream_t st = nullptr;
  int status = BP_OK;
  std::string why;
  char buf[384];
  // the members' own constraints, as bp_check_txn_witness reports a table's
  for (uint32_t t = 0; t < n_tables; t++) {
    bp_set_table_report& o = out->table[t];
    const bp_stark_cfg& c = tables[t].cfg;
    uint32_t rows[8], nv = 0;
    if ((rc = bp_air_check_trace(tables[t].air_id, &c, tables[t].d_trace, tables[t].stride, sh.cfg[t].n_const ? tables[t].d_consts : nullptr,
                                 tables[t].pub, 8, &o.n_violated_rows, rows, o.viol, 8, &nv, st))) return rc;
    o.n_viol = std::min<uint32_t>(nv, 8);
    if (status == BP_OK && o.n_violated_rows) {
      std::snprintf(buf, sizeof(buf), "table %u does not satisfy its AIR: row %u violates constraint %u (family %u), %llu rows in all", t,
                    o.viol[0].row, o.viol[0].constraint, o.viol[0].family, (unsigned long long)o.n_violated_rows);
      status = BP_ERR_VERIFY;
      why = buf;
    }
  }
  // the links: one scratch for the largest, reused link after link; a link's eight result words behind the slots
  uint32_t log_slots[SET_MAX_LINKS], max_log = 0;
  for (uint32_t k = 0; k < n_links; k++) {
    uint64_t rows = 0;
    for (uint32_t m = 0; m <= links[k].n_looking; m++)
      rows += (uint64_t)1 << sh.cfg[(m < links[k].n_looking ? links[k].looking[m] : links[k].looked).table].log_n;
    log_slots[k] = set_check_log_slots(rows);
    max_log = std::max(max_log, log_slots[k]);
  }
  const size_t table_words = ((size_t)1 << max_log) * SET_SLOT_WORDS, bytes = (table_words + (size_t)SET_RESULT_WORDS * n_links) * 8;
  uint64_t* d_s = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&d_s), bytes) != hipSuccess) {
    (void)hipGetLastError();
    return fail(BP_ERR_DEVICE, "bp_check_table_set: the device has no %zu bytes for the balance of the largest link", bytes);
  }
  struct Free { void* p; ~Free() { (void)hipFree(p); } } guard{d_s};
  std::random_device rd;
  std::mt19937_64 g(((uint64_t)rd() << 32) ^ rd());
  uint64_t ctl[4];
  for (uint64_t& v : ctl) do v = g() % gl::P; while (v < 2);
  auto end_of = [&](const bp_set_link& l, uint32_t m) {
    const bp_set_port& e = m < l.n_looking ? l.looking[m] : l.looked;
    const bp_set_table& tb = tables[e.table];
    SetEnd se{};
    se.air_id = tb.air_id; se.port = e.port;
    se.trace = tb.d_trace; se.consts = sh.cfg[e.table].n_const ? tb.d_consts : nullptr; se.stride = tb.stride;
    se.log_n = sh.cfg[e.table].log_n;
    if (tb.pub) for (int j = 0; j < 4; j++) se.pub[j] = tb.pub[j];
    se.end = m; se.looked = m == l.n_looking;
    // a port that demands a bit: a registered program's product port or kind-1 log port (a built-in member's own AIR
    // constrains its filter; a kind-2 filter is a multiplicity)
    const auto program = air::prog::find(tb.air_id);
    se.wants_bit = program && e.port < program->n_ports && program->port_kind[e.port] != air::prog::PORT_LOG_MULT;
    return se;
  };
  for (uint32_t k = 0; k < n_links; k++) {
    SetEnd ends[SET_MAX_LOOKING + 1];
    for (uint32_t m = 0; m <= links[k].n_looking; m++) ends[m] = end_of(links[k], m);
    if ((rc = launch_set_link(ends, links[k].n_looking + 1, ctl, d_s, log_slots[k], d_s + table_words + (size_t)SET_RESULT_WORDS * k, st))) return rc;
  }
  uint64_t res[SET_MAX_LINKS][SET_RESULT_WORDS];
  BPG_HIP(hipMemcpyAsync(res, d_s + table_words, (size_t)SET_RESULT_WORDS * n_links * 8, hipMemcpyDeviceToHost, st));
  BPG_HIP(hipStreamSynchronize(st));
  const uint64_t row_mask = ((uint64_t)1 << SET_LOC_ROW_BITS) - 1;
  for (uint32_t k = 0; k < n_links; k++) {
    const bp_set_link& l = links[k];
    bp_set_link_report& o = out->link[k];
    const uint64_t* r = res[k];
    if (r[SET_RES_OVERFLOW]) return fail(BP_ERR_DEVICE, "bp_check_table_set: link %u: the balance table overflowed", k);
    o.is_log = sh.log_link[k];
    o.n_looking = r[SET_RES_N_LOOKING];
    o.n_looked = r[SET_RES_N_LOOKED];
    o.n_unbalanced = r[SET_RES_UNBALANCED];
    o.first_looking_end = o.bad_filter_end = -1;
    o.first_looking_row = o.first_looked_row = o.bad_filter_row = -1;
    if (r[SET_RES_MIN_LOOKING] != ~0ULL) {
      o.first_looking_end = (int32_t)(r[SET_RES_MIN_LOOKING] >> SET_LOC_ROW_BITS);
      o.first_looking_row = (int64_t)(r[SET_RES_MIN_LOOKING] & row_mask);
    }
    if (r[SET_RES_MIN_LOOKED] != ~0ULL) o.first_looked_row = (int64_t)r[SET_RES_MIN_LOOKED];
    if (r[SET_RES_BAD_FILTER] != ~0ULL) {
      o.bad_filter_end = (int32_t)(r[SET_RES_BAD_FILTER] >> SET_LOC_ROW_BITS);
      o.bad_filter_row = (int64_t)(r[SET_RES_BAD_FILTER] & row_mask);
      uint64_t* d_res = d_s + table_words + (size_t)SET_RESULT_WORDS * k;
      if ((rc = launch_set_filter_at(end_of(l, (uint32_t)o.bad_filter_end), (uint64_t)o.bad_filter_row, ctl, d_res, st))) return rc;
      BPG_HIP(hipMemcpyAsync(&o.bad_filter_value, d_res + SET_RES_BAD_VALUE, 8, hipMemcpyDeviceToHost, st));
      BPG_HIP(hipStreamSynchronize(st));
    }
    o.holds = o.n_unbalanced == 0 && o.bad_filter_end < 0;
    if (status != BP_OK || o.holds) continue;
    status = BP_ERR_VERIFY;
    if (o.bad_filter_end >= 0) {
      const bp_set_port& e = (uint32_t)o.bad_filter_end < l.n_looking ? l.looking[o.bad_filter_end] : l.looked;
      std::snprintf(buf, sizeof(buf), "link %u: the filter of port %u of table %u is no bit on row %lld: it is %llu", k, e.port, e.table,
                    (long long)o.bad_filter_row, (unsigned long long)o.bad_filter_value);
    } else {
      const bp_set_port& e = l.looking[o.first_looking_end < 0 ? 0 : o.first_looking_end];
      std::snprintf(buf, sizeof(buf), "link %u does not balance (%llu tuple values): first unmatched looking row %lld (port %u of table %u), "
                    "looked row %lld (port %u of table %u)", k, (unsigned long long)o.n_unbalanced, (long long)o.first_looking_row, e.port, e.table,
                    (long long)o.first_looked_row, l.looked.port, l.looked.table);
    }
    why = buf;
  }
  return status == BP_OK ? BP_OK : fail(status, "%s", why.c_str());
}
BPG_ABI_CATCH("bp_check_table_set")

}  // extern "C"

extern "C" {

void bp_free_buffer(uint8_t* buf) { std::free(buf); }
// Host only: the transcript's CPU permutation (prover.cpp, poseidon_host) over n states of 12 words, in place.
int bp_debug_poseidon_host(uint64_t* states, size_t n) try {
  if (!states && n) return bpg::fail(BP_ERR_INVALID_INPUT, "bp_debug_poseidon_host: null states");
  for (size_t i = 0; i < n; i++) bpg::poseidon_host(states + 12 * i);
  return BP_OK;
}
BPG_ABI_CATCH("bp_debug_poseidon_host")

void bp_release_cached_memory(void) {
  std::vector<Worker*> all;
  {
    std::lock_guard<std::mutex> lk(g_park_mu);
    all.swap(g_parked);
  }
  for (Worker* w : all)
    if (w) {
      w->destroy();
      delete w;
    }
}

int bp_stark_prove_air(uint32_t air_id, const bp_stark_cfg* cfg, uint64_t seed, uint64_t const_seed, int device,
                       uint8_t** out, size_t* out_len) try {
  if (!cfg || !out || !out_len) return fail(BP_ERR_INVALID_INPUT, "bp_stark_prove_air: null argument");
  if (air::prog::is_registered(air_id))
    return fail(BP_ERR_INVALID_INPUT, "bp_stark_prove_air: a registered AIR has no witness generator to draw from a seed: prove its trace "
                "with bp_stark_prove_trace");
  StarkCfg c{cfg->log_n, cfg->n_cols, cfg->n_const, cfg->deg_pow, cfg->rate_bits, cfg->cap_height,
             cfg->num_queries, cfg->pow_bits, cfg->arity_bits, cfg->final_poly_bits, air_id};
  int rc = check_cfg(c);
  if (rc) return rc;
  const uint64_t N = (uint64_t)1 << c.log_n, M = N << c.rate_bits;
  // generous one-shot arena: every oracle (values + coeffs + LDE) plus temporaries
  const size_t cols = (size_t)c.n_cols + c.n_const + c.n_cols / 8 + (2u << c.rate_bits) + 64;
  size_t bytes = cols * (2 * N + M) * 8 + (size_t)80 * M * 8 + ((size_t)c.n_cols / 32 + 64) * 8 * N * 8 + (64u << 20);
  Worker* wp = take_worker(device, bytes, &rc);
  if (!wp) return rc;
  Worker& w = *wp;
  // parked again (or freed) on every way out, an exception included: the worker holds the arena
  struct Parker {
    Worker* w;
    ~Parker() { park_worker(w); }
  } parker{wp};
  auto body = [&]() -> int {
    Challenger ch;
    Committed consts, trace;
    uint64_t* d_consts = nullptr;
    if (c.n_const) {
      d_consts = w.arena.alloc_words((size_t)c.n_const * N);
      if (!d_consts) return fail(BP_ERR_DEVICE, "arena exhausted");
      int r2 = c.air_id == air::PLONK ? launch_plonk_constants(d_consts, c.log_n, const_seed, air::plonk::Layout{LONE_PI_LEN, 0, 0, 0}, w.stream)
                                      : launch_synth_constants(d_consts, c.log_n, c.n_const, const_seed, w.stream);
      if (r2) return r2;
      if ((r2 = commit(w, d_consts, c.n_const, c.log_n, c.rate_bits, c.cap_height, false, &consts))) return r2;
      ch.observe(consts.cap.data(), consts.cap.size());
    }
    uint64_t* d_trace = w.arena.alloc_words((size_t)c.n_cols * N);
    if (!d_trace) return fail(BP_ERR_DEVICE, "arena exhausted");
    int r2 = c.air_id == air::PLONK ? BP_OK  // (its witness needs the public inputs: below)
             : c.air_id == air::SYNTHETIC ? launch_synth_trace(d_trace, d_consts, c.log_n, c.n_cols, c.n_const, c.deg_pow, seed, w.stream)
                                          : launch_air_trace(c.air_id, d_trace, nullptr, c.log_n, seed, w.stream);
    Ctl ctl;
    if (c.air_id == air::PLONK) {  // the public-input list of a lone table proof follows from the seed (lone_public_input_list)
      uint64_t pi[LONE_PI_LEN];
      lone_public_input_list(seed, pi);
      std::vector<uint64_t> rows;
      poseidon_hash_rows(pi, LONE_PI_LEN, &rows, ctl.pub);   // the circuit hashes the list in its hash rows: pub = that hash
      std::memcpy(w.hash_rows, rows.data(), rows.size() * 8);
      PlonkTraceArgs pa{d_trace, d_consts, seed, {ctl.pub[0], ctl.pub[1], ctl.pub[2], ctl.pub[3]}, w.hash_rows_dev, 1};
      r2 = launch_plonk_trace(&pa, 1, c.log_n, w.stream);
    }
    if (r2) return r2;
    if ((r2 = commit(w, d_trace, c.n_cols, c.log_n, c.rate_bits, c.cap_height, false, &trace))) return r2;
    ch.observe(trace.cap.data(), trace.cap.size());
    for (int i = 0; i < 4; i++) ctl.v[i] = ch.challenge();
    std::vector<uint64_t> proof;
    if ((r2 = stark_prove(w, c, c.n_const ? &consts : nullptr, trace, d_trace, ctl, ch, proof))) return r2;
    *out_len = proof.size() * 8;
    *out = static_cast<uint8_t*>(std::malloc(*out_len));
    if (!*out) return fail(BP_ERR_DEVICE, "host allocation failed");
    std::memcpy(*out, proof.data(), *out_len);
    return BP_OK;
  };
  rc = body();
  // nothing of this call is still in flight when the worker is parked (a failed call keeps its own message)
  if (rc) (void)hipStreamSynchronize(w.stream);
  else rc = w.wait();
  return rc;
}
BPG_ABI_CATCH("bp_stark_prove_air")

// The same proof from the caller's trace: what bp_stark_prove_air does after its witness generator has run.
int bp_stark_prove_trace(uint32_t air_id, const bp_stark_cfg* cfg, const uint64_t* d_trace, uint64_t stride, const uint64_t* d_consts,
                         const uint64_t* pub, int device, uint8_t** out, size_t* out_len) try {
  if (!cfg || !d_trace || !out || !out_len) return fail(BP_ERR_INVALID_INPUT, "bp_stark_prove_trace: null argument");
  StarkCfg c{cfg->log_n, cfg->n_cols, cfg->n_const, cfg->deg_pow, cfg->rate_bits, cfg->cap_height,
             cfg->num_queries, cfg->pow_bits, cfg->arity_bits, cfg->final_poly_bits, air_id};
  int rc = check_cfg(c);
  if (rc) return rc;
  const uint64_t N = (uint64_t)1 << c.log_n, M = N << c.rate_bits;
  if (stride < N) return fail(BP_ERR_INVALID_INPUT, "bp_stark_prove_trace: column stride %llu is shorter than the %llu-row trace",
                              (unsigned long long)stride, (unsigned long long)N);
  if (c.n_const && !d_consts) return fail(BP_ERR_INVALID_INPUT, "bp_stark_prove_trace: the AIR reads %u constant columns: pass them", c.n_const);
  const auto program = air::prog::find(air_id);
  Ctl ctl;
  if (air_id == air::PLONK || (program && program->n_public)) {
    if (!pub) return fail(BP_ERR_INVALID_INPUT, "bp_stark_prove_trace: the AIR reads public inputs: pass four words");
    for (int j = 0; j < 4; j++) {
      if (pub[j] >= gl::P) return fail(BP_ERR_INVALID_INPUT, "bp_stark_prove_trace: non-canonical public input");
      ctl.pub[j] = pub[j];
    }
  }
  // the arena of bp_stark_prove_air, plus the trace itself when it has to be packed to stride n
  const size_t cols = (size_t)c.n_cols + c.n_const + c.n_cols / 8 + (2u << c.rate_bits) + 64;
  size_t bytes = cols * (2 * N + M) * 8 + (size_t)80 * M * 8 + ((size_t)c.n_cols / 32 + 64) * 8 * N * 8 + (64u << 20);
  if (stride != N) bytes += (size_t)c.n_cols * N * 8;
  Worker* wp = take_worker(device, bytes, &rc);
  if (!wp) return rc;
  Worker& w = *wp;
  struct Parker {
    Worker* w;
    ~Parker() { park_worker(w); }
  } parker{wp};
  auto body = [&]() -> int {
    Challenger ch;
    Committed consts, trace;
    if (c.n_const) {
      int r2 = commit(w, d_consts, c.n_const, c.log_n, c.rate_bits, c.cap_height, false, &consts);
      if (r2) return r2;
      ch.observe(consts.cap.data(), consts.cap.size());
    }
    const uint64_t* d_tv = d_trace;
    if (stride != N) {
      uint64_t* packed = w.arena.alloc_words((size_t)c.n_cols * N);
      if (!packed) return fail(BP_ERR_DEVICE, "arena exhausted");
      BPG_HIP(hipMemcpy2DAsync(packed, N * 8, d_trace, stride * 8, N * 8, c.n_cols, hipMemcpyDeviceToDevice, w.stream));
      d_tv = packed;
    }
    int r2 = commit(w, d_tv, c.n_cols, c.log_n, c.rate_bits, c.cap_height, false, &trace);
    if (r2) return r2;
    ch.observe(trace.cap.data(), trace.cap.size());
    for (int i = 0; i < 4; i++) ctl.v[i] = ch.challenge();
    std::vector<uint64_t> proof;
    if ((r2 = stark_prove(w, c, c.n_const ? &consts : nullptr, trace, d_tv, ctl, ch, proof))) return r2;
    *out_len = proof.size() * 8;
    *out = static_cast<uint8_t*>(std::malloc(*out_len));
    if (!*out) return fail(BP_ERR_DEVICE, "host allocation failed");
    std::memcpy(*out, proof.data(), *out_len);
    return BP_OK;
  };
  rc = body();
  if (rc) (void)hipStreamSynchronize(w.stream);
  else if ((rc = w.wait())) {  // the caller gets no buffer with a failure
    std::free(*out);
    *out = nullptr;
    *out_len = 0;
  }
  return rc;
}
BPG_ABI_CATCH("bp_stark_prove_trace")

int bp_stark_prove_synthetic(const bp_stark_cfg* cfg, uint64_t seed, uint64_t const_seed, int device,
                             uint8_t** out, size_t* out_len) {
  return bp_stark_prove_air(air::SYNTHETIC, cfg, seed, const_seed, device, out, out_len);
}

// The CPU verifier for one table proof of bp_stark_prove_air (same transcript prologue: constants cap if any, trace
// cap, four CTL challenges).  Host only: runs without a GPU.
// A lone AIR-8 table proof made from `seed` has the public-input LIST splitmix64(seed ^ ((0x50 + j) << 32)) mod p, j < 4
// (in a transaction the list is child digests and public values); the four public inputs bound to its first row are the
// hash of that list, which the circuit computes in its hash rows and the verifier computes for itself.
void bp_stark_public_input_list(uint64_t seed, uint64_t out[4]) { lone_public_input_list(seed, out); }
void bp_stark_public_inputs(uint64_t seed, uint64_t out[4]) {
  uint64_t pi[LONE_PI_LEN];
  lone_public_input_list(seed, pi);
  hash_no_pad_host(pi, LONE_PI_LEN, out);
}

int bp_stark_verify_air(uint32_t air_id, const bp_stark_cfg* cfg, const uint64_t* const_cap, const uint8_t* proof,
                        size_t len) {
  return bp_stark_verify_air_pub(air_id, cfg, const_cap, nullptr, proof, len);
}
int bp_stark_verify_air_pub(uint32_t air_id, const bp_stark_cfg* cfg, const uint64_t* const_cap, const uint64_t* pub,
                            const uint8_t* proof, size_t len) try {
  if (!cfg || !proof) return fail(BP_ERR_INVALID_INPUT, "bp_stark_verify_air: null argument");
  StarkCfg c{cfg->log_n, cfg->n_cols, cfg->n_const, cfg->deg_pow, cfg->rate_bits, cfg->cap_height,
             cfg->num_queries, cfg->pow_bits, cfg->arity_bits, cfg->final_poly_bits, air_id};
  int rc = check_cfg(c);
  if (rc) return rc;
  if (c.n_const && !const_cap) return fail(BP_ERR_INVALID_INPUT, "bp_stark_verify_air: the table has constant columns: pass their cap");
  const ProofLayout L = proof_layout(c);
  if (len != L.total * 8) return fail(BP_ERR_VERIFY, "proof has %zu bytes, expected %zu", len, L.total * 8);
  std::vector<uint64_t> w(L.total);
  std::memcpy(w.data(), proof, len);
  Challenger ch;
  if (c.n_const) ch.observe(const_cap, L.cap_words);
  ch.observe(w.data() + L.trace_cap, L.cap_words);
  Ctl ctl;
  for (int i = 0; i < 4; i++) ctl.v[i] = ch.challenge();
  if (pub)
    for (int i = 0; i < 4; i++) {
      if (pub[i] >= gl::P) return fail(BP_ERR_INVALID_INPUT, "non-canonical public input");
      ctl.pub[i] = pub[i];
    }
  return stark_verify(c, c.n_const ? const_cap : nullptr, ctl, ch, w.data(), w.size());
}
BPG_ABI_CATCH("bp_stark_verify_air_pub")

// ---- the AIR registry (air.hpp) --------------------------------------------------------------------------

// the BUILT-IN AIRs only: registered programs (air_program.cpp) live beside them under ids with the top bit set
uint32_t bp_air_count(void) { return air::COUNT; }

int bp_air_describe(uint32_t air_id, uint32_t n_cols, uint32_t n_const, uint32_t deg_pow, bp_air_desc* out) try {
  if (const auto p = air::prog::find(air_id)) {  // a registered program answers from its own tables; the width asked about is ignored
    if (!out) return fail(BP_ERR_INVALID_INPUT, "bp_air_describe: null output");
    std::memset(out, 0, sizeof(*out));
    out->air_id = air_id;
    std::strncpy(out->name, "program", sizeof(out->name) - 1);
    out->fixed_n_cols = out->n_cols = p->n_cols;
    out->n_const_max = p->n_const;
    out->degree = p->degree;
    // without ports "a table no lookup is built for": the constant running product AIR 4 and AIR 7 have
    out->n_aux = p->n_aux();
    out->n_air_constraints = p->n_constraints;
    out->n_ctl_constraints = p->n_ctl_constraints();
    out->n_units = p->n_units;
    uint32_t n = 0;
    for (uint32_t f = 0; f < p->n_families; f++)
      out->families[n++] = bp_air_family{p->families[f].first_index, p->families[f].count, p->families[f].kind, p->families[f].degree};
    if (!p->n_ports) {
      if (n < 24) out->families[n++] = bp_air_family{p->n_constraints, 1, 1, 3};
      if (n < 24) out->families[n++] = bp_air_family{p->n_constraints + 1, 1, 3, 2};
    }
    // per port: the filter bit, then per challenge set the running column's transition and last-row constraint, with the
    // degrees registration propagated (air_program.hpp): a product port's z - z' term and z - term, a log port's
    // (s - s') d - f and s d - f, whose bit slot is identically zero when the filter is a multiplicity.  Where five
    // families per port do not fit the description, three interleaved ones stand for all ports (period 5: the bits at
    // b + 5l, the transitions at b + 5l + 1 and + 3, the last-row ones at b + 5l + 2 and + 4), with the largest degree
    // among the ports.
    auto port_degrees = [&](uint32_t l, uint32_t* bit, uint32_t* step, uint32_t* last) {
      const uint32_t df = p->port_deg_f[l], dt = p->port_deg_t[l];
      *bit = p->port_kind[l] == air::prog::PORT_LOG_MULT ? 1 : std::max(1u, 2 * df);
      if (p->port_kind[l] != air::prog::PORT_PRODUCT) {
        *step = *last = std::max(1 + dt, df);
      } else {
        *step = 1 + df + dt;
        *last = std::max(1u, df + dt);
      }
    };
    if (n + air::prog::PORT_CONSTRAINTS * p->n_ports > 24) {
      uint32_t d0 = 1, d1 = 1, d2 = 1;
      for (uint32_t l = 0; l < p->n_ports; l++) {
        uint32_t bit, step, last;
        port_degrees(l, &bit, &step, &last);
        d0 = std::max(d0, bit);
        d1 = std::max(d1, step);
        d2 = std::max(d2, last);
      }
      out->families[n++] = bp_air_family{p->n_constraints, p->n_ports, 0, d0};
      out->families[n++] = bp_air_family{p->n_constraints + 1, 2 * p->n_ports, 1, d1};
      out->families[n++] = bp_air_family{p->n_constraints + 2, 2 * p->n_ports, 3, d2};
    } else
    for (uint32_t l = 0; l < p->n_ports; l++) {
      const uint32_t b = p->n_constraints + air::prog::PORT_CONSTRAINTS * l;
      uint32_t bit, step, last;
      port_degrees(l, &bit, &step, &last);
      out->families[n++] = bp_air_family{b, 1, 0, bit};
      for (uint32_t c = 0; c < 2; c++) {
        out->families[n++] = bp_air_family{b + 1 + 2 * c, 1, 1, step};
        out->families[n++] = bp_air_family{b + 2 + 2 * c, 1, 3, last};
      }
    }
    out->n_families = n;
    return BP_OK;
  }
  const air::Desc* ai = air::info(air_id);
  if (!ai || !out) return fail(BP_ERR_INVALID_INPUT, "bp_air_describe: unknown air_id %u or null output", air_id);
  std::memset(out, 0, sizeof(*out));
  out->air_id = air_id;
  std::strncpy(out->name, ai->name, sizeof(out->name) - 1);
  out->fixed_n_cols = ai->n_cols;
  out->n_const_max = ai->n_const_max;
  const uint32_t C = ai->n_cols ? ai->n_cols : n_cols, dp = ai->n_cols ? (ai->degree > 3 ? 3 : 1) : (deg_pow ? deg_pow : 1);
  const air::Shape shape{air_id, C, ai->n_cols ? ai->n_const_max : n_const, dp};
  out->degree = ai->n_cols ? ai->degree : ai->degree * dp;
  out->n_cols = C;
  out->n_aux = air::ctl::n_aux(shape);
  out->n_air_constraints = air::n_constraints(shape);
  out->n_ctl_constraints = air::ctl::n_constraints(shape);
  out->n_units = air::n_units(shape);
  // families: (first index, count, kind, degree); kinds: 0 all rows, 1 transition, 2 first row, 3 last row
  uint32_t n = 0;
  auto fam = [&](uint32_t first, uint32_t count, uint32_t kind, uint32_t degree) {
    if (n < 24) out->families[n++] = bp_air_family{first, count, kind, degree};
  };
  // the AIR's own constraints, then the table's lookups (air::ctl) in list order after them
  const uint32_t b = out->n_air_constraints;
  if (air_id == air::SYNTHETIC) {
    // interleaved per group of four columns: 3g all rows, 3g + 1 transition, 3g + 2 first row
    fam(0, C / 4, 0, 2); fam(1, C / 4, 1, 3 * dp); fam(2, C / 4, 2, 1);
    fam(b, C / 8, 1, 2); fam(b + 1, C / 8, 3, 1);  // running products, interleaved 2k (transition), 2k + 1 (last row)
  } else {
    for (const air::Family& f : ai->families) if (f.count) fam(f.first, f.count, f.kind, f.degree);
    for (const air::Family& f : ai->ctl_families) if (f.count) fam(b + f.first, f.count, f.kind, f.degree);
  }
  out->n_families = n;
  return BP_OK;
}
BPG_ABI_CATCH("bp_air_describe")

// the seven bp_<table>_trace entries: one body, the table's name in the messages
static int table_trace(const char* entry, uint32_t air_id, const uint64_t* d_inputs, uint64_t seed, uint32_t log_n, uint64_t* d_trace_out,
                       void* stream) {
  if (!d_trace_out) return fail(BP_ERR_INVALID_INPUT, "%s: null output", entry);
  if (log_n < 4 || log_n > 26) return fail(BP_ERR_INVALID_INPUT, "%s: log_n out of range", entry);
  return launch_air_trace(air_id, d_trace_out, d_inputs, log_n, seed, as_stream(stream));
}
int bp_keccak_trace(const uint64_t* d_inputs, uint64_t seed, uint32_t log_n, uint64_t* d_trace_out, void* stream) try {
  return table_trace("bp_keccak_trace", air::KECCAK_F, d_inputs, seed, log_n, d_trace_out, stream);
}
BPG_ABI_CATCH("bp_keccak_trace")
int bp_logic_trace(const uint64_t* d_inputs, uint64_t seed, uint32_t log_n, uint64_t* d_trace_out, void* stream) try {
  return table_trace("bp_logic_trace", air::LOGIC, d_inputs, seed, log_n, d_trace_out, stream);
}
BPG_ABI_CATCH("bp_logic_trace")
int bp_memory_trace(const uint64_t* d_inputs, uint64_t seed, uint32_t log_n, uint64_t* d_trace_out, void* stream) try {
  return table_trace("bp_memory_trace", air::MEMORY, d_inputs, seed, log_n, d_trace_out, stream);
}
BPG_ABI_CATCH("bp_memory_trace")
int bp_arithmetic_trace(const uint64_t* d_inputs, uint64_t seed, uint32_t log_n, uint64_t* d_trace_out, void* stream) try {
  return table_trace("bp_arithmetic_trace", air::ARITHMETIC, d_inputs, seed, log_n, d_trace_out, stream);
}
BPG_ABI_CATCH("bp_arithmetic_trace")
int bp_byte_packing_trace(const uint64_t* d_inputs, uint64_t seed, uint32_t log_n, uint64_t* d_trace_out, void* stream) try {
  return table_trace("bp_byte_packing_trace", air::BYTE_PACKING, d_inputs, seed, log_n, d_trace_out, stream);
}
BPG_ABI_CATCH("bp_byte_packing_trace")
int bp_keccak_sponge_trace(const uint64_t* d_inputs, uint64_t seed, uint32_t log_n, uint64_t* d_trace_out, void* stream) try {
  return table_trace("bp_keccak_sponge_trace", air::KECCAK_SPONGE, d_inputs, seed, log_n, d_trace_out, stream);
}
BPG_ABI_CATCH("bp_keccak_sponge_trace")
int bp_arithmetic_mul_trace(const uint64_t* d_inputs, uint64_t seed, uint32_t log_n, uint64_t* d_trace_out, void* stream) try {
  return table_trace("bp_arithmetic_mul_trace", air::ARITHMETIC_MUL, d_inputs, seed, log_n, d_trace_out, stream);
}
BPG_ABI_CATCH("bp_arithmetic_mul_trace")

// AIR 8: the preprocessed constants of the fixed PLONK-shaped circuit (85 columns: selectors, gate constants drawn from
// `seed`, the hash-row selector, sigmas) for a circuit that hashes a public-input list of pi_len words, and its witness
// (135 wires; free wires drawn from `seed`; the list pi is hashed in the hash rows, the hash lands in row 0).
static int plonk_layout_of(const bp_plonk_layout* l, uint32_t log_n, air::plonk::Layout* out) {
  if (!l) return fail(BP_ERR_INVALID_INPUT, "null plonk layout");
  *out = air::plonk::Layout{l->pi_len, l->n_paths, l->path_depth, l->path_pi0, l->leaf_len};
  if (!air::plonk::layout_ok(*out, 1u << log_n))
    return fail(BP_ERR_INVALID_INPUT, "plonk layout: a list of 1..%u words, at most %u Merkle rows (n_paths x path_depth), the paths' words "
                "(8 per path from path_pi0) inside the list, and room for one arithmetic group in 2^%u rows", air::plonk::MAX_PI,
                air::plonk::MERKLE_ROWS_MAX, log_n);
  return BP_OK;
}
int bp_plonk_constants(uint64_t seed, uint32_t log_n, const bp_plonk_layout* layout, uint64_t* d_consts_out, void* stream) try {
  if (!d_consts_out) return fail(BP_ERR_INVALID_INPUT, "bp_plonk_constants: null output");
  if (log_n < 4 || log_n > 26) return fail(BP_ERR_INVALID_INPUT, "bp_plonk_constants: log_n out of range");
  air::plonk::Layout lay;
  int rc = plonk_layout_of(layout, log_n, &lay);
  if (rc) return rc;
  if ((rc = init_ntt_kernels())) return rc;
  return launch_plonk_constants(d_consts_out, log_n, seed, lay, as_stream(stream));
}
BPG_ABI_CATCH("bp_plonk_constants")
int bp_plonk_trace(const uint64_t* d_consts, uint64_t seed, const uint64_t* pi, const bp_plonk_layout* layout, const uint64_t* paths,
                   uint32_t log_n, uint64_t* d_trace_out, void* stream) try {
  if (!d_consts || !pi || !d_trace_out) return fail(BP_ERR_INVALID_INPUT, "bp_plonk_trace: null argument");
  if (log_n < 4 || log_n > 26) return fail(BP_ERR_INVALID_INPUT, "bp_plonk_trace: log_n out of range");
  air::plonk::Layout lay;
  int rc = plonk_layout_of(layout, log_n, &lay);
  if (rc) return rc;
  if (lay.n_paths && !paths) return fail(BP_ERR_INVALID_INPUT, "bp_plonk_trace: the layout walks %u Merkle paths: their witness is missing", lay.n_paths);
  for (uint32_t j = 0; j < lay.pi_len; j++) if (pi[j] >= gl::P) return fail(BP_ERR_INVALID_INPUT, "bp_plonk_trace: non-canonical public input");
  std::vector<uint64_t> rows, all((size_t)(air::plonk::HASH_ROWS_MAX + air::plonk::merkle_rows(lay) + air::plonk::leaf_rows(lay)) * air::plonk::H_WIRES, 0);
  uint64_t pub[4];
  poseidon_hash_rows(pi, lay.pi_len, &rows, pub);
  std::memcpy(all.data(), rows.data(), rows.size() * 8);
  const uint32_t n_list_rows = (uint32_t)(rows.size() / air::plonk::H_WIRES);
  const size_t path_words = 1 + 4 * (size_t)lay.depth + lay.leaf_len;
  for (uint32_t p = 0; p < lay.n_paths; p++) {
    const uint64_t* pw = paths + p * path_words;
    for (size_t j = 1; j < path_words; j++) if (pw[j] >= gl::P) return fail(BP_ERR_INVALID_INPUT, "bp_plonk_trace: non-canonical sibling word");
    uint64_t root[4];
    poseidon_merkle_rows(pi + lay.path_pi0 + 8 * p, pw[0], pw + 1, lay.depth,
                         all.data() + (size_t)(air::plonk::HASH_ROWS_MAX + p * lay.depth) * air::plonk::H_WIRES, root);
    if (lay.leaf_len) {
      uint64_t digest[4];
      poseidon_hash_rows(pw + 1 + 4 * (size_t)lay.depth, lay.leaf_len, &rows, digest);
      std::memcpy(all.data() + (size_t)(air::plonk::HASH_ROWS_MAX + air::plonk::merkle_rows(lay) + p * air::plonk::hash_rows(lay.leaf_len)) * air::plonk::H_WIRES,
                  rows.data(), rows.size() * 8);
    }
  }
  // (a test / integration entry: the rows go up with a blocking copy into a buffer of their own)
  uint64_t* d_rows = nullptr;
  BPG_HIP(hipMalloc(reinterpret_cast<void**>(&d_rows), all.size() * 8));
  struct Free { uint64_t* p; ~Free() { (void)hipFree(p); } } guard{d_rows};
  BPG_HIP(hipMemcpy(d_rows, all.data(), all.size() * 8, hipMemcpyHostToDevice));
  PlonkTraceArgs a{d_trace_out, d_consts, seed, {pub[0], pub[1], pub[2], pub[3]}, d_rows, n_list_rows,
                   air::plonk::merkle_rows(lay) + air::plonk::leaf_rows(lay), air::plonk::arith_row0(lay)};
  rc = launch_plonk_trace(&a, 1, log_n, as_stream(stream));
  if (rc) return rc;
  BPG_HIP(hipStreamSynchronize(as_stream(stream)));
  return BP_OK;
}
BPG_ABI_CATCH("bp_plonk_trace")

// ---- L0: the remaining per-stage entry points of SURVEY.md section 8(b) -------------------------------

static int quot_cfg(uint32_t air_id, const bp_stark_cfg* shape, StarkCfg* c) {
  if (!shape) return fail(BP_ERR_INVALID_INPUT, "null shape");
  *c = StarkCfg{shape->log_n, shape->n_cols, shape->n_const, shape->deg_pow, shape->rate_bits, shape->cap_height,
                shape->num_queries, shape->pow_bits, shape->arity_bits, shape->final_poly_bits, air_id};
  return check_cfg(*c);
}

uint64_t bp_quotient_scratch_words(uint32_t air_id, const bp_stark_cfg* shape) {
  StarkCfg c;
  if (quot_cfg(air_id, shape, &c)) return 0;
  // The spreading of the units over workgroup rows follows the device's load, which bp_generate_* calls on other
  // threads change at any moment: the scratch is sized for the larger of the two forms (the unloaded one spreads
  // furthest), so a launch that finds another load state than this call did still fits.
  QuotArgs qa{};
  Ctl ctl{};
  if (init_ntt_kernels()) return 0;
  uint64_t words = 0;
  for (int loaded = 0; loaded < 2; loaded++) {
    if (quotient_args(c, ctl, 1, 1, &qa, nullptr, loaded)) return 0;
    words = std::max<uint64_t>(words, quotient_table_words(qa) + quotient_partial_words(qa));
  }
  return words;
}

int bp_quotient_eval(uint32_t air_id, const bp_stark_cfg* shape, const uint64_t* d_trace_lde, const uint64_t* d_aux_lde,
                     const uint64_t* d_const_lde, const uint64_t ctl_in[4], const uint64_t alphas[2],
                     uint64_t* d_scratch, uint64_t* d_qvals_out, void* stream) try {
  StarkCfg c;
  int rc = quot_cfg(air_id, shape, &c);
  if (rc) return rc;
  if (!d_trace_lde || !d_aux_lde || (c.n_const && !d_const_lde) || !ctl_in || !alphas || !d_scratch || !d_qvals_out)
    return fail(BP_ERR_INVALID_INPUT, "bp_quotient_eval: null argument");
  for (int i = 0; i < 4; i++)
    if (ctl_in[i] >= gl::P) return fail(BP_ERR_INVALID_INPUT, "bp_quotient_eval: non-canonical challenge");
  if (alphas[0] >= gl::P || alphas[1] >= gl::P) return fail(BP_ERR_INVALID_INPUT, "bp_quotient_eval: non-canonical alpha");
  if ((rc = init_ntt_kernels())) return rc;
  Ctl ctl;
  for (int i = 0; i < 4; i++) ctl.v[i] = ctl_in[i];
  QuotArgs qa{};
  QuotCoset coset{};
  qa.trace_lde = d_trace_lde; qa.aux_lde = d_aux_lde; qa.const_lde = c.n_const ? d_const_lde : nullptr;
  if ((rc = quotient_args(c, ctl, alphas[0], alphas[1], &qa, &coset))) return rc;
  qa.apow = d_scratch; qa.partial = d_scratch + quotient_table_words(qa); qa.qvals = d_qvals_out;
  return launch_quotient(qa, coset, as_stream(stream));
}
BPG_ABI_CATCH("bp_quotient_eval")

// The running products of a registered program's ports on the trace domain: what stark_prove commits as the table's
// auxiliary columns, without a proof around it.
int bp_air_port_products(uint32_t air_id, const bp_stark_cfg* shape, const uint64_t* d_trace, uint64_t stride, const uint64_t* d_consts,
                         const uint64_t pub[4], const uint64_t ctl_in[4], uint64_t* d_aux_out, void* stream) try {
  const auto program = air::prog::find(air_id);
  if (!program || !program->n_ports)
    return fail(BP_ERR_INVALID_INPUT, "bp_air_port_products: air_id 0x%08x is no registered program with lookup ports", air_id);
  StarkCfg c;
  int rc = quot_cfg(air_id, shape, &c);
  if (rc) return rc;
  if (!d_trace || !ctl_in || !d_aux_out || (c.n_const && !d_consts)) return fail(BP_ERR_INVALID_INPUT, "bp_air_port_products: null argument");
  if (stride < ((uint64_t)1 << c.log_n))
    return fail(BP_ERR_INVALID_INPUT, "bp_air_port_products: column stride %llu is shorter than the 2^%u-row trace", (unsigned long long)stride, c.log_n);
  AuxArgs a{d_trace, d_aux_out, Ctl{}};
  a.consts = c.n_const ? d_consts : nullptr;
  for (int i = 0; i < 4; i++) {
    if (ctl_in[i] >= gl::P || (pub && pub[i] >= gl::P)) return fail(BP_ERR_INVALID_INPUT, "bp_air_port_products: non-canonical challenge or public input");
    a.ctl.v[i] = ctl_in[i];
    a.ctl.pub[i] = pub ? pub[i] : 0;
  }
  if (program->n_public && !pub) return fail(BP_ERR_INVALID_INPUT, "bp_air_port_products: the AIR reads public inputs: pass four words");
  return launch_port_products(&a, 1, air_id, c.log_n, stride, as_stream(stream));
}
BPG_ABI_CATCH("bp_air_port_products")

// Test entry: the auxiliary columns (helpers and running products, bp_air_desc.n_aux of them, column stride 2^log_n) the
// prover commits for a BUILT-IN table with a lookup side, from a trace of column stride 2^log_n.
int bp_debug_air_aux(uint32_t air_id, const bp_stark_cfg* shape, const uint64_t* d_trace, const uint64_t ctl_in[4], uint64_t* d_aux_out,
                     void* stream) try {
  const air::Desc* ai = air::info(air_id);
  if (!ai || !ai->in_pair) return fail(BP_ERR_INVALID_INPUT, "bp_debug_air_aux: air_id %u is no built-in AIR with a lookup side", air_id);
  StarkCfg c;
  int rc = quot_cfg(air_id, shape, &c);
  if (rc) return rc;
  if (!d_trace || !ctl_in || !d_aux_out) return fail(BP_ERR_INVALID_INPUT, "bp_debug_air_aux: null argument");
  AuxArgs a{d_trace, d_aux_out, Ctl{}};
  for (int i = 0; i < 4; i++) {
    if (ctl_in[i] >= gl::P) return fail(BP_ERR_INVALID_INPUT, "bp_debug_air_aux: non-canonical challenge");
    a.ctl.v[i] = ctl_in[i];
  }
  return launch_aux(&a, 1, air_id, c.n_cols, c.log_n, as_stream(stream));
}
BPG_ABI_CATCH("bp_debug_air_aux")

int bp_fri_fold(const uint64_t* d_values, uint32_t log_nl, uint32_t rate_bits, uint32_t arity_bits, uint64_t shift,
                const uint64_t beta[2], uint64_t* d_out, void* stream) try {
  if (!d_values || !d_out || !beta) return fail(BP_ERR_INVALID_INPUT, "bp_fri_fold: null argument");
  if (shift == 0 || shift >= gl::P || beta[0] >= gl::P || beta[1] >= gl::P)
    return fail(BP_ERR_INVALID_INPUT, "bp_fri_fold: non-canonical field element");
  int rc = init_ntt_kernels();
  if (rc) return rc;
  FriLayerArgs fa{};
  if ((rc = fri_layer_args(log_nl, rate_bits, arity_bits, shift, &fa))) return rc;
  fa.values = d_values; fa.out = d_out; fa.digests = nullptr;
  fa.beta = gl::Ext{beta[0], beta[1]};
  return launch_fri_fold(fa, as_stream(stream));
}
BPG_ABI_CATCH("bp_fri_fold")

int bp_pow_grind(const uint64_t state[12], uint32_t pos, uint32_t bits, uint64_t* nonce_out, void* stream) try {
  if (!state || !nonce_out) return fail(BP_ERR_INVALID_INPUT, "bp_pow_grind: null argument");
  if (pos >= 8 || bits == 0 || bits > 40) return fail(BP_ERR_INVALID_INPUT, "bp_pow_grind: pos must be a rate word, bits in 1..40");
  hipStream_t st = as_stream(stream);
  unsigned long long* d_res = nullptr;
  BPG_HIP(hipMalloc(reinterpret_cast<void**>(&d_res), 8));
  PowArgs pa{};
  for (int i = 0; i < 12; i++) pa.state[i] = state[i];
  pa.pos = pos; pa.bits = bits;
  int rc = BP_OK;
  unsigned long long res = ~0ULL;
  if (hipMemsetAsync(d_res, 0xFF, 8, st) != hipSuccess) rc = fail(BP_ERR_DEVICE, "hipMemsetAsync failed");
  uint32_t batch = (uint32_t)std::min<uint64_t>(1u << 20, std::max<uint64_t>(1u << 12, (uint64_t)2 << bits));
  for (uint64_t base = 0; rc == BP_OK; base += batch, batch = std::min<uint32_t>(1u << 20, batch * 2)) {
    pa.base = base;
    if ((rc = launch_pow(pa, batch, d_res, st))) break;
    if (hipMemcpyAsync(&res, d_res, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
      rc = fail(BP_ERR_DEVICE, "bp_pow_grind: copy back failed");
      break;
    }
    if (res != ~0ULL) break;
    if (base > ((uint64_t)1 << 44)) rc = fail(BP_ERR_DEVICE, "proof of work search exhausted");
  }
  (void)hipFree(d_res);
  if (rc == BP_OK) *nonce_out = res;
  return rc;
}
BPG_ABI_CATCH("bp_pow_grind")

int bp_openings(const uint64_t* d_coeffs, uint64_t stride, uint32_t log_n, uint32_t n_cols, const uint64_t z0[2],
                const uint64_t z1[2], uint64_t* d_pw_scratch, uint64_t* d_out, void* stream) try {
  if (!n_cols) return BP_OK;
  if (!d_coeffs || !z0 || !d_pw_scratch || !d_out) return fail(BP_ERR_INVALID_INPUT, "bp_openings: null argument");
  if (log_n > 30 || stride < ((uint64_t)1 << log_n)) return fail(BP_ERR_INVALID_INPUT, "bp_openings: bad shape");
  const uint64_t* zz[2] = {z0, z1 ? z1 : z0};
  for (int k = 0; k < 2; k++)
    if (zz[k][0] >= gl::P || zz[k][1] >= gl::P) return fail(BP_ERR_INVALID_INPUT, "bp_openings: non-canonical point");
  hipStream_t st = as_stream(stream);
  const uint32_t n_points = z1 ? 2 : 1;
  int rc = launch_power_vectors(d_pw_scratch, log_n, gl::Ext{z0[0], z0[1]}, gl::Ext{zz[1][0], zz[1][1]}, n_points, st);
  if (rc) return rc;
  return launch_openings(d_coeffs, stride, log_n, n_cols, d_pw_scratch, n_points, d_out, st);
}
BPG_ABI_CATCH("bp_openings")

}  // extern "C"
