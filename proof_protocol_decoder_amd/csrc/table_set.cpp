// table_set.cpp -- table sets: several caller traces linked port to port, proven on one transcript (include/bpg.h):
// the statement and its refusals (check_set), what both sides observe of it (observe_set), and the entries
// bp_stark_prove_table_set, bp_stark_verify_table_set, bp_check_table_set.  Below the statement, and shared with a
// transaction's seven tables (txn_tables.cpp, proofgen.cpp): the links on the first-row openings (first_failing_link) and
// the pre-flight of tables and links (check_tables_and_links).
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>
#include "caller_table.hpp"
#include "set_check.hpp"

using namespace bpg;

namespace {
constexpr uint64_t SET_MAGIC = 0x3154455354475042ULL;  // "BPGTSET1"
constexpr uint32_t SET_MAX_TABLES = 8, SET_MAX_LINKS = 16, SET_MAX_LOOKING = 8;

// the lookup ports of a member: a registered program's own, a built-in's product columns in air::DESC order
// (port l = columns first_product + 2l + c); 0: the id is no side of any lookup
uint32_t set_ports_of(uint32_t air_id) {
  if (const auto p = air::prog::find(air_id)) return p->n_ports;
  const air::Desc* d = air::info(air_id);
  if (!d || !d->in_pair) return 0;
  return (d->n_aux - d->first_product) / 2;
}
struct Where {  // "table %u: " in front of what is refused about a member
  char s[24];
  explicit Where(uint32_t t) { std::snprintf(s, sizeof(s), "table %u: ", t); }
};
struct SetShape {
  CallerTable table[SET_MAX_TABLES];  // (the verifier's statement leaves the device pointers alone)
  StarkCfg cfgs[SET_MAX_TABLES];      // table[t].cfg, side by side as first_failing_link reads them
  const StarkCfg& cfg(uint32_t t) const { return cfgs[t]; }
  uint32_t n_ports[SET_MAX_TABLES];
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
    const bp_set_table& m = tables[t];
    const CallerTable& tb = out->table[t] = caller_table(to_cfg(m.cfg, m.air_id), m.d_trace, m.stride, m.d_consts, m.pub);
    out->cfgs[t] = tb.cfg;
    if (int rc = check_cfg(tb.cfg)) {
      const std::string why = bp_last_error();
      return fail(rc, "%s: table %u: %s", who, t, why.c_str());
    }
    out->n_ports[t] = set_ports_of(m.air_id);
    out->log_ports[t] = tb.program ? tb.program->log_ports() : 0;  // a built-in member's ports are product ports
    if (!out->n_ports[t])
      return fail(BP_ERR_INVALID_INPUT, "%s: table %u: air_id %u (0x%08x) has no lookup port: a member is a registered program with ports or "
                  "one of the built-in AIRs 1, 2, 3, 5, 6", who, t, tables[t].air_id, tables[t].air_id);
    if (int rc = check_public_inputs(who, Where(t).s, tb)) return rc;
  }
  for (uint32_t k = 0; k < n_links; k++) {
    const bp_set_link& l = links[k];
    if (l.n_looking < 1 || l.n_looking > SET_MAX_LOOKING)
      return fail(BP_ERR_INVALID_INPUT, "%s: link %u has %u looking ports (1 .. %u)", who, k, l.n_looking, SET_MAX_LOOKING);
    for (uint32_t m = 0; m <= l.n_looking; m++) {
      const bp_set_port& e = link_end(l, m);
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
// what the entries that read the traces refuse about the members, after the statement's refusals and before any device call
int check_set_tables(const char* who, const SetShape& sh, uint32_t n_tables) {
  for (uint32_t t = 0; t < n_tables; t++)
    if (int rc = check_caller_table(who, Where(t).s, sh.table[t])) return rc;
  return BP_OK;
}
// the statement, as both sides observe it before any commitment
int observe_set(Challenger& ch, const bp_set_table* tables, uint32_t n_tables, const bp_set_link* links, uint32_t n_links, const SetShape& sh) {
  ch.observe(SET_MAGIC % gl::P);
  ch.observe(n_tables);
  ch.observe(n_links);
  for (uint32_t t = 0; t < n_tables; t++) {
    const StarkCfg& c = sh.cfg(t);
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
      const bp_set_port& e = link_end(links[k], m);
      ch.observe(e.table);
      ch.observe(e.port);
    }
  }
  return BP_OK;
}
// Every link on the first-row openings (first_failing_link), in a set's words
int check_links(const SetShape& sh, const bp_set_link* links, uint32_t n_links, const std::vector<uint64_t>* proof) {
  uint32_t k, c;
  if (!first_failing_link(sh.cfgs, proof, links, sh.log_link, n_links, &k, &c)) return BP_OK;
  const bp_set_link& l = links[k];
  return fail(BP_ERR_VERIFY, "link %u does not hold (challenge set %u): port %u of table %u%s asks for tuples that port %u of table %u "
              "does not expose", k, c, l.looking[0].port, l.looking[0].table, l.n_looking > 1 ? " (and the link's other looking ports)" : "",
              l.looked.port, l.looked.table);
}
}  // namespace

namespace bpg {

bool first_failing_link(const StarkCfg* cfg, const std::vector<uint64_t>* proof, const bp_set_link* links, const bool* log_link,
                        uint32_t n_links, uint32_t* link, uint32_t* set) {
  for (uint32_t k = 0; k < n_links; k++) {
    const bp_set_link& l = links[k];
    const bool is_log = log_link && log_link[k];
    for (uint32_t c = 0; c < 2; c++) {
      auto first_row = [&](const bp_set_port& e) {  // (a registered program's products start at column 0)
        const uint64_t* v = proof[e.table].data() + proof_layout(cfg[e.table]).open_first +
                            2 * (size_t)(air::ctl::first_product(cfg[e.table].air_id) + 2 * e.port + c);
        return gl::Ext{v[0], v[1]};
      };
      gl::Ext a = gl::ext(is_log ? 0 : 1);
      for (uint32_t m = 0; m < l.n_looking; m++) a = is_log ? gl::add(a, first_row(l.looking[m])) : gl::mul(a, first_row(l.looking[m]));
      const gl::Ext b = first_row(l.looked);
      if (a.c0 != b.c0 || a.c1 != b.c1) {
        *link = k;
        *set = c;
        return true;
      }
    }
  }
  return false;
}

int check_tables_and_links(const char* who, const CallerTable* tables, uint32_t n_tables, const bp_set_link* links, const bool* log_link,
                           uint32_t n_links, hipStream_t st, bp_set_table_report* table, bp_set_link_report* link) {
  int rc;
  for (uint32_t t = 0; t < n_tables; t++) {
    const CallerTable& tb = tables[t];
    if (!tb.trace) continue;
    bp_set_table_report& o = table[t];
    const bp_stark_cfg shape = abi_cfg(tb.cfg);
    uint32_t rows[8], nv = 0;
    if ((rc = bp_air_check_trace(tb.cfg.air_id, &shape, tb.trace, tb.stride, tb.consts, tb.pub, 8, &o.n_violated_rows, rows, o.viol, 8, &nv,
                                 st))) return rc;
    o.n_viol = std::min<uint32_t>(nv, 8);
  }
  if (!n_links) return BP_OK;
  // the links: one scratch for the largest, reused link after link; a link's eight result words behind the slots
  uint32_t log_slots[SET_MAX_LINKS], max_log = 0;
  for (uint32_t k = 0; k < n_links; k++) {
    uint64_t rows = 0;
    for (uint32_t m = 0; m <= links[k].n_looking; m++)
      rows += (uint64_t)1 << tables[link_end(links[k], m).table].cfg.log_n;
    log_slots[k] = set_check_log_slots(rows);
    max_log = std::max(max_log, log_slots[k]);
  }
  const size_t table_words = ((size_t)1 << max_log) * SET_SLOT_WORDS, bytes = (table_words + (size_t)SET_RESULT_WORDS * n_links) * 8;
  DeviceBuf scratch;
  if (hipMalloc(&scratch.p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    return fail(BP_ERR_DEVICE, "%s: the device has no %zu bytes for the balance of the largest link", who, bytes);
  }
  uint64_t* d_s = scratch.as<uint64_t>();
  FreshChallenges fresh;
  uint64_t ctl[4];
  for (uint64_t& v : ctl) v = fresh();
  auto end_of = [&](const bp_set_link& l, uint32_t m) {
    const bp_set_port& e = link_end(l, m);
    const CallerTable& tb = tables[e.table];
    SetEnd se{};
    se.air_id = tb.cfg.air_id; se.port = e.port;
    se.trace = tb.trace; se.consts = tb.consts; se.stride = tb.stride;
    se.log_n = tb.cfg.log_n;
    if (tb.pub) for (int j = 0; j < 4; j++) se.pub[j] = tb.pub[j];
    se.end = m; se.looked = m == l.n_looking;
    // a port that demands a bit: a registered program's product port or kind-1 log port (a built-in member's own AIR
    // constrains its filter; a kind-2 filter is a multiplicity)
    se.wants_bit = tb.program && e.port < tb.program->n_ports && tb.program->port_kind[e.port] != air::prog::PORT_LOG_MULT;
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
    bp_set_link_report& o = link[k];
    const uint64_t* r = res[k];
    if (r[SET_RES_OVERFLOW]) return fail(BP_ERR_DEVICE, "%s: link %u: the balance table overflowed", who, k);
    o.is_log = log_link && log_link[k];
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
      if ((rc = launch_set_filter_at(end_of(links[k], (uint32_t)o.bad_filter_end), (uint64_t)o.bad_filter_row, ctl, d_res, st))) return rc;
      BPG_HIP(hipMemcpyAsync(&o.bad_filter_value, d_res + SET_RES_BAD_VALUE, 8, hipMemcpyDeviceToHost, st));
      BPG_HIP(hipStreamSynchronize(st));
    }
    o.holds = o.n_unbalanced == 0 && o.bad_filter_end < 0;
  }
  return BP_OK;
}

}  // namespace bpg

extern "C" {

int bp_stark_prove_table_set(const bp_set_table* tables, uint32_t n_tables, const bp_set_link* links, uint32_t n_links, uint32_t flags,
                             int device, uint8_t** out, size_t* out_len) try {
  if (!out || !out_len) return fail(BP_ERR_INVALID_INPUT, "bp_stark_prove_table_set: null argument");
  if (flags & ~(uint32_t)BP_SET_SKIP_LINK_CHECK) return fail(BP_ERR_INVALID_INPUT, "bp_stark_prove_table_set: unknown flags 0x%x", flags);
  SetShape sh;
  int rc = check_set("bp_stark_prove_table_set", tables, n_tables, links, n_links, &sh);
  if (rc) return rc;
  if ((rc = check_set_tables("bp_stark_prove_table_set", sh, n_tables))) return rc;
  size_t bytes = ARENA_SLACK;
  for (uint32_t t = 0; t < n_tables; t++) bytes += table_arena_bytes(sh.cfg(t), sh.table[t].stride != (uint64_t)1 << sh.cfg(t).log_n);
  WorkerLease lease(device, bytes);
  if (lease.rc()) return lease.rc();
  Worker& w = *lease;
  auto body = [&]() -> int {
    Challenger ch;
    int r2 = observe_set(ch, tables, n_tables, links, n_links, sh);
    if (r2) return r2;
    // every commitment before the lookup challenges exist: per table the constants (if any), the trace, the public inputs
    Committed consts[SET_MAX_TABLES], trace[SET_MAX_TABLES];
    const uint64_t* d_tv[SET_MAX_TABLES];
    Ctl ctl[SET_MAX_TABLES];
    for (uint32_t t = 0; t < n_tables; t++) {
      if ((r2 = commit_caller_table(w, ch, sh.table[t], &consts[t], &trace[t], &d_tv[t]))) return r2;
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
      if ((r2 = stark_prove(w, sh.cfg(t), sh.cfg(t).n_const ? &consts[t] : nullptr, trace[t], d_tv[t], ctl[t], ch, proof[t]))) return r2;
      w.arena.release(mark);
    }
    if (!(flags & BP_SET_SKIP_LINK_CHECK))
      if ((r2 = check_links(sh, links, n_links, proof))) return r2;
    std::vector<uint64_t> blob = {SET_MAGIC, n_tables, n_links, v[0], v[1], v[2], v[3]};
    for (uint32_t k = 0; k < n_links; k++) {
      blob.push_back(links[k].n_looking);
      for (uint32_t m = 0; m <= links[k].n_looking; m++) {
        const bp_set_port& e = link_end(links[k], m);
        blob.push_back(e.table);
        blob.push_back(e.port);
      }
    }
    for (uint32_t t = 0; t < n_tables; t++) {
      const uint64_t hdr[4] = {sh.cfg(t).air_id, sh.cfg(t).log_n, sh.cfg(t).n_cols, proof[t].size()};
      blob.insert(blob.end(), hdr, hdr + 4);
      blob.insert(blob.end(), proof[t].begin(), proof[t].end());
    }
    return emit(blob, out, out_len);
  };
  return finish(w, body(), out, out_len);
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
    if (sh.cfg(t).n_const && !(const_caps && const_caps[t]))
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
      const bp_set_port& e = link_end(l, m);
      same = W[off + 1 + 2 * m] == e.table && W[off + 2 + 2 * m] == e.port;
    }
    if (!same) return fail(BP_ERR_VERIFY, "table set: link %u of the container is not link %u of the statement", k, k);
    off += 3 + 2 * (size_t)l.n_looking;
  }
  std::vector<uint64_t> proof[SET_MAX_TABLES];
  ProofLayout L[SET_MAX_TABLES];
  for (uint32_t t = 0; t < n_tables; t++) {
    const StarkCfg& c = sh.cfg(t);
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
    if (sh.cfg(t).n_const) ch.observe(const_caps[t], L[t].cap_words);
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
    if ((rc = stark_verify(sh.cfg(t), sh.cfg(t).n_const ? const_caps[t] : nullptr, ctl[t], ch, proof[t].data(), proof[t].size()))) {
      const std::string why = bp_last_error();
      return fail(rc, "table set: table %u: %s", t, why.c_str());
    }
  return check_links(sh, links, n_links, proof);
}
BPG_ABI_CATCH("bp_stark_verify_table_set")

// The pre-flight of a set (include/bpg.h): check_tables_and_links behind the statement's refusals, on the null stream.
// Nothing is committed or proven; every table and every link is reported.
int bp_check_table_set(const bp_set_table* tables, uint32_t n_tables, const bp_set_link* links, uint32_t n_links, int device,
                       bp_set_report* out) try {
  if (!out) return fail(BP_ERR_INVALID_INPUT, "bp_check_table_set: null argument");
  SetShape sh;
  int rc = check_set("bp_check_table_set", tables, n_tables, links, n_links, &sh);
  if (rc) return rc;
  if ((rc = check_set_tables("bp_check_table_set", sh, n_tables))) return rc;
  std::memset(out, 0, sizeof(*out));
  int before = 0;
  BPG_HIP(hipGetDevice(&before));
  BPG_HIP(hipSetDevice(device));
  struct Back { int d; ~Back() { (void)hipSetDevice(d); } } back{before};
  if ((rc = check_tables_and_links("bp_check_table_set", sh.table, n_tables, links, sh.log_link, n_links, nullptr, out->table, out->link)))
    return rc;
  // the first finding: tables in index order (as bp_check_txn_witness words a table's), then links
  for (uint32_t t = 0; t < n_tables; t++) {
    const bp_set_table_report& o = out->table[t];
    if (o.n_violated_rows)
      return fail(BP_ERR_VERIFY, "table %u does not satisfy its AIR: row %u violates constraint %u (family %u), %llu rows in all", t,
                  o.viol[0].row, o.viol[0].constraint, o.viol[0].family, (unsigned long long)o.n_violated_rows);
  }
  for (uint32_t k = 0; k < n_links; k++) {
    const bp_set_link& l = links[k];
    const bp_set_link_report& o = out->link[k];
    if (o.holds) continue;
    if (o.bad_filter_end >= 0) {
      const bp_set_port& e = link_end(l, (uint32_t)o.bad_filter_end);
      return fail(BP_ERR_VERIFY, "link %u: the filter of port %u of table %u is no bit on row %lld: it is %llu", k, e.port, e.table,
                  (long long)o.bad_filter_row, (unsigned long long)o.bad_filter_value);
    }
    const bp_set_port& e = l.looking[o.first_looking_end < 0 ? 0 : o.first_looking_end];
    return fail(BP_ERR_VERIFY, "link %u does not balance (%llu tuple values): first unmatched looking row %lld (port %u of table %u), "
                "looked row %lld (port %u of table %u)", k, (unsigned long long)o.n_unbalanced, (long long)o.first_looking_row, e.port, e.table,
                (long long)o.first_looked_row, l.looked.port, l.looked.table);
  }
  return BP_OK;
}
BPG_ABI_CATCH("bp_check_table_set")

}  // extern "C"
