// stark_api.cpp -- the C ABI of the lone table proofs (bp_stark_prove_air from a seed, bp_stark_prove_trace from the
// caller's trace, their CPU verifier), of the AIR registry (bp_air_describe, the witness generators) and of the L0
// per-stage entries (include/bpg.h).  Table sets are table_set.cpp's; what is shared about a caller's table,
// caller_table.hpp's.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "caller_table.hpp"
#include "plonk_hash_fold.hpp"

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
// One table proof on a transcript of its own: the constants cap (if any), the trace cap, four challenges, the proof.
int prove_lone(Worker& w, const CallerTable& t, uint8_t** out, size_t* out_len) {
  Challenger ch;
  Committed consts, trace;
  const uint64_t* d_values = nullptr;
  int rc = commit_caller_table(w, ch, t, &consts, &trace, &d_values);
  if (rc) return rc;
  Ctl ctl;
  if (t.pub)
    for (int j = 0; j < 4; j++) ctl.pub[j] = t.pub[j];
  for (int i = 0; i < 4; i++) ctl.v[i] = ch.challenge();
  std::vector<uint64_t> proof;
  if ((rc = stark_prove(w, t.cfg, t.cfg.n_const ? &consts : nullptr, trace, d_values, ctl, ch, proof))) return rc;
  return emit(proof, out, out_len);
}
}  // namespace

extern "C" {

void bp_free_buffer(uint8_t* buf) { std::free(buf); }
// Host only: the transcript's CPU permutation (prover.cpp, poseidon_host) over n states of 12 words, in place.
int bp_debug_poseidon_host(uint64_t* states, size_t n) try {
  if (!states && n) return bpg::fail(BP_ERR_INVALID_INPUT, "bp_debug_poseidon_host: null states");
  for (size_t i = 0; i < n; i++) bpg::poseidon_host(states + 12 * i);
  return BP_OK;
}
BPG_ABI_CATCH("bp_debug_poseidon_host")

// AIR 8's fold block (plonk_hash_fold.hpp) for one pair of challenges: as the quotient's launch makes it on the device,
// and by the recurrences on the host.
static int hash_fold_alphas(const char* who, const uint64_t alphas[2], const void* out) {
  if (!alphas || !out) return bpg::fail(BP_ERR_INVALID_INPUT, "%s: null argument", who);
  if (alphas[0] >= gl::P || alphas[1] >= gl::P) return bpg::fail(BP_ERR_INVALID_INPUT, "%s: non-canonical alpha", who);
  return BP_OK;
}
int bp_debug_plonk_hash_fold(const uint64_t alphas[2], uint64_t* d_out, void* stream) try {
  if (int rc = hash_fold_alphas("bp_debug_plonk_hash_fold", alphas, d_out)) return rc;
  if (int rc = init_ntt_kernels()) return rc;
  return debug_plonk_hash_fold(alphas[0], alphas[1], d_out, as_stream(stream));
}
BPG_ABI_CATCH("bp_debug_plonk_hash_fold")
int bp_debug_plonk_hash_fold_host(const uint64_t alphas[2], uint64_t* out) try {
  if (int rc = hash_fold_alphas("bp_debug_plonk_hash_fold_host", alphas, out)) return rc;
  uint64_t block[air::plonk::HASH_FOLD_WORDS];
  air::plonk::hash_fold_block_host(air::plonk::N_CONSTRAINTS + air::ctl::PLONK_N_CONSTRAINTS, alphas[0], alphas[1], block);
  std::memcpy(out, block, sizeof(block));
  return BP_OK;
}
BPG_ABI_CATCH("bp_debug_plonk_hash_fold_host")

void bp_release_cached_memory(void) { release_parked_workers(); }

// The witness generator of a built-in AIR fills the arena with constants and trace; the rest is bp_stark_prove_trace's.
int bp_stark_prove_air(uint32_t air_id, const bp_stark_cfg* cfg, uint64_t seed, uint64_t const_seed, int device,
                       uint8_t** out, size_t* out_len) try {
  if (!cfg || !out || !out_len) return fail(BP_ERR_INVALID_INPUT, "bp_stark_prove_air: null argument");
  if (air::prog::is_registered(air_id))
    return fail(BP_ERR_INVALID_INPUT, "bp_stark_prove_air: a registered AIR has no witness generator to draw from a seed: prove its trace "
                "with bp_stark_prove_trace");
  const StarkCfg c = to_cfg(*cfg, air_id);
  int rc = check_cfg(c);
  if (rc) return rc;
  const uint64_t N = (uint64_t)1 << c.log_n;
  WorkerLease lease(device, table_arena_bytes(c, false) + ARENA_SLACK);
  if (lease.rc()) return lease.rc();
  Worker& w = *lease;
  auto body = [&]() -> int {
    uint64_t* d_consts = c.n_const ? w.arena.alloc_words((size_t)c.n_const * N) : nullptr;
    uint64_t* d_trace = w.arena.alloc_words((size_t)c.n_cols * N);
    if (!d_trace || (c.n_const && !d_consts)) return fail(BP_ERR_DEVICE, "arena exhausted");
    uint64_t pub[4];
    int r2 = BP_OK;
    if (c.air_id == air::PLONK) {  // the public-input list of a lone table proof follows from the seed (lone_public_input_list)
      if ((r2 = launch_plonk_constants(d_consts, c.log_n, const_seed, air::plonk::Layout{LONE_PI_LEN, 0, 0, 0}, w.stream))) return r2;
      uint64_t pi[LONE_PI_LEN];
      lone_public_input_list(seed, pi);
      std::vector<uint64_t> rows;
      poseidon_hash_rows(pi, LONE_PI_LEN, &rows, pub);   // the circuit hashes the list in its hash rows: pub = that hash
      std::memcpy(w.hash_rows, rows.data(), rows.size() * 8);
      PlonkTraceArgs pa{d_trace, d_consts, seed, {pub[0], pub[1], pub[2], pub[3]}, w.hash_rows_dev, 1};
      r2 = launch_plonk_trace(&pa, 1, c.log_n, w.stream);
    } else {
      if (c.n_const && (r2 = launch_synth_constants(d_consts, c.log_n, c.n_const, const_seed, w.stream))) return r2;
      r2 = c.air_id == air::SYNTHETIC ? launch_synth_trace(d_trace, d_consts, c.log_n, c.n_cols, c.n_const, c.deg_pow, seed, w.stream)
                                      : launch_air_trace(c.air_id, d_trace, nullptr, c.log_n, seed, w.stream);
    }
    if (r2) return r2;
    return prove_lone(w, caller_table(c, d_trace, N, d_consts, c.air_id == air::PLONK ? pub : nullptr), out, out_len);
  };
  return finish(w, body(), out, out_len);
}
BPG_ABI_CATCH("bp_stark_prove_air")

// The same proof from the caller's trace.
int bp_stark_prove_trace(uint32_t air_id, const bp_stark_cfg* cfg, const uint64_t* d_trace, uint64_t stride, const uint64_t* d_consts,
                         const uint64_t* pub, int device, uint8_t** out, size_t* out_len) try {
  if (!cfg || !out || !out_len) return fail(BP_ERR_INVALID_INPUT, "bp_stark_prove_trace: null argument");
  const StarkCfg c = to_cfg(*cfg, air_id);
  int rc = check_cfg(c);
  if (rc) return rc;
  CallerTable t = caller_table(c, d_trace, stride, d_consts, pub);
  if (!t.reads_public()) t.pub = nullptr;  // public inputs the AIR does not read are not looked at
  if ((rc = check_caller_table("bp_stark_prove_trace", "", t))) return rc;
  WorkerLease lease(device, table_arena_bytes(c, stride != (uint64_t)1 << c.log_n) + ARENA_SLACK);
  if (lease.rc()) return lease.rc();
  return finish(*lease, prove_lone(*lease, t, out, out_len), out, out_len);
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
  const StarkCfg c = to_cfg(*cfg, air_id);
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
  DeviceBuf rows_buf;
  BPG_HIP(hipMalloc(&rows_buf.p, all.size() * 8));
  uint64_t* d_rows = rows_buf.as<uint64_t>();
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
  *c = to_cfg(*shape, air_id);
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
  if (!ctl_in || !d_aux_out) return fail(BP_ERR_INVALID_INPUT, "bp_air_port_products: null argument");
  const CallerTable t = caller_table(c, d_trace, stride, d_consts, pub);
  if ((rc = check_caller_table("bp_air_port_products", "", t))) return rc;
  AuxArgs a{d_trace, d_aux_out, Ctl{}};
  a.consts = t.consts;
  for (int i = 0; i < 4; i++) {
    if (ctl_in[i] >= gl::P) return fail(BP_ERR_INVALID_INPUT, "bp_air_port_products: non-canonical challenge");
    a.ctl.v[i] = ctl_in[i];
    a.ctl.pub[i] = pub ? pub[i] : 0;
  }
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
  DeviceBuf res_buf;
  BPG_HIP(hipMalloc(&res_buf.p, 8));
  unsigned long long* d_res = res_buf.as<unsigned long long>();
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
