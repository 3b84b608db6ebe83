// txn_tables.cpp -- the host-only code over the descriptor of a transaction's seven tables (txn_tables.hpp).
#include <algorithm>
#include <string>
#include "caller_table.hpp"
#include "txn_tables.hpp"

namespace bpg {
namespace txn {

void root_after(const uint64_t root_before[4], uint64_t seed, uint64_t txn_number, uint64_t out[4]) {
  uint64_t in[6] = {root_before[0], root_before[1], root_before[2], root_before[3], gl::canon(seed), gl::canon(txn_number)};
  hash_no_pad_host(in, 6, out);
}
int ir_set_air(uint64_t ir[BP_IR_WORDS], int t, int which, int on) {
  const Table& T = TABLES[t];
  const TableAir& a = T.airs[which];
  if (!ir || ir[0] != IR_MAGIC) return fail(BP_ERR_INVALID_INPUT, "%s: not an IR", a.setter);
  if (on && ir[18 + t] != air::DESC[a.air_id].n_cols)
    return fail(BP_ERR_INVALID_INPUT, "the %s AIR has %u columns: the IR gives table %s %llu", a.noun, air::DESC[a.air_id].n_cols, T.name,
                (unsigned long long)ir[18 + t]);
  for (int k = 0; on && k < which; k++)
    if (ir[1] & T.airs[k].ir_mask) return fail(BP_ERR_INVALID_INPUT, "the %s table is proven by ONE AIR: clear %s first", T.name, T.airs[k].setter);
  ir[1] = (ir[1] & ~a.ir_mask) | (on ? a.ir_mask : 0);
  return BP_OK;
}
void TxnWitness::give(int t, const uint64_t* p, size_t count) {
  static const uint64_t none = 0;
  in[t] = p ? p : &none;
  n[t] = count;
}
int witness_of(const bp_txn_witness* data, TxnWitness* wit) {
  for (int t = 0; data && t < BP_NUM_TABLES; t++) {
    const Table& T = TABLES[t];
    if (!T.has || !(data->*T.has)) continue;
    if (!(data->*T.data) && data->*T.n) return fail(BP_ERR_INVALID_INPUT, "bp_generate_txn_proof_witness: null data for table %s", T.name);
    wit->give(t, data->*T.data, data->*T.n);
  }
  return BP_OK;
}
void fill_table_inputs(int t, uint64_t N, const uint64_t* in, size_t n, uint64_t* dst) {
  const size_t cap = witness_capacity(t, N), wds = TABLES[t].item_words;
  std::memcpy(dst, in, n * wds * 8);
  std::memset(dst + n * wds, 0, (cap - n) * wds * 8);
  if (t == T_MEMORY) {  // keep reading the last cell (a first-row read of zero memory when the log is empty)
    uint64_t last[TABLES[T_MEMORY].item_words] = {1};
    if (n) std::memcpy(last, in + (n - 1) * wds, sizeof(last));
    last[0] = 1;
    for (size_t i = n; i < cap; i++) {
      last[2] += 1;
      std::memcpy(dst + i * wds, last, sizeof(last));
    }
  }
}
bool given_table(const TxnWitness* wit, const StarkCfg tcfg[BP_NUM_TABLES], int t) {
  return wit && wit->in[t] && table_has_air(t, tcfg[t].air_id);
}
int parse_ir(const bp_config& cfg, const uint64_t* I, const TxnWitness* wit, StarkCfg tcfg[BP_NUM_TABLES], std::vector<uint64_t>* pv_out) {
  // word 1: the version byte -- 1: a transaction; 2: a dummy entry (decoding.rs:484-520): txn number, gas and state
  // root do not advance, the same tables are proven -- and above it the flags that prove a table with one of its AIRs
  // (TABLES[t].airs; include/bpg.h lists them) instead of the synthetic one
  uint64_t ver = I[1] & 0xFF, known = 0xFF;
  for (const Table& T : TABLES) known |= T.airs[0].ir_mask | T.airs[1].ir_mask;
  if (I[0] != IR_MAGIC || (ver != 1 && ver != 2) || (I[1] & ~known)) return fail(BP_ERR_INVALID_INPUT, "IR: bad magic/version");
  for (const Table& T : TABLES)
    if ((I[1] & T.airs[0].ir_mask) && (I[1] & T.airs[1].ir_mask))
      return fail(BP_ERR_INVALID_INPUT, "IR: the %s table is proven by ONE AIR (flags 0x%llx and 0x%llx are both set)", T.name,
                  (unsigned long long)T.airs[0].ir_mask, (unsigned long long)T.airs[1].ir_mask);
  const bool dummy = ver == 2;
  if (wit) {
    for (int t = 0; t < BP_NUM_TABLES; t++) {
      if (!wit->in[t]) continue;
      if (!air_selected(t, I[1]))
        return fail(BP_ERR_INVALID_INPUT, "witness data for table %s needs an IR whose %s table is proven with its AIR (bp_ir_set_*_air)",
                    TABLES[t].name, TABLES[t].name);
      if (I[11 + t] < 40 && wit->n[t] > witness_capacity(t, (uint64_t)1 << I[11 + t]))
        return fail(BP_ERR_RANGE, "%zu witness items do not fit table %s of 2^%llu rows%s", wit->n[t], TABLES[t].name,
                    (unsigned long long)I[11 + t], t == T_KECCAK ? " (24 rows per Keccak permutation)" : "");
    }
  }
  if (I[5] < I[4]) return fail(BP_ERR_INVALID_INPUT, "IR: gas_used_after < gas_used_before");
  if (dummy && I[5] != I[4]) return fail(BP_ERR_INVALID_INPUT, "IR: a dummy entry must not use gas (decoding.rs:503-506)");
  for (int t = 0; t < BP_NUM_TABLES; t++) {
    const uint64_t ln = I[11 + t], wd = I[18 + t];
    if (ln < cfg.table_log_lo[t] || ln >= cfg.table_log_hi[t])
      return fail(BP_ERR_RANGE, "table %s needs 2^%llu rows, outside the configured range %u..%u", TABLES[t].name,
                  (unsigned long long)ln, cfg.table_log_lo[t], cfg.table_log_hi[t]);
    if (wd > 65536) return fail(BP_ERR_INVALID_INPUT, "table %s: width out of range", TABLES[t].name);
    tcfg[t] = table_cfg_of(cfg, (uint32_t)ln, (uint32_t)wd);
    if (const TableAir* a = air_selected(t, I[1])) tcfg[t].air_id = a->air_id;  // check_cfg insists on the AIR's own width
    int r = check_cfg(tcfg[t]);
    if (r) return r;
  }
  for (int i = 0; i < 4; i++) if (I[6 + i] >= gl::P) return fail(BP_ERR_INVALID_INPUT, "IR: non-canonical state root");
  // PublicValues
  std::vector<uint64_t>& pv = *pv_out;
  pv.assign(BP_PV_WORDS, 0);
  pv[0] = I[3]; pv[1] = I[3] + (dummy ? 0 : 1); pv[2] = I[4]; pv[3] = I[5];
  std::memcpy(&pv[4], I + 6, 32);
  if (dummy) std::memcpy(&pv[8], I + 6, 32);
  else root_after(I + 6, I[10], I[3], &pv[8]);
  pv[12] = I[2];
  for (auto& v : pv) v = gl::canon(v);
  return BP_OK;
}
int plan_traces(const StarkCfg tcfg[BP_NUM_TABLES], const bool given[BP_NUM_TABLES], const size_t n_given[BP_NUM_TABLES], TracePlan* out) {
  const air::ctl::Pair* P = air::ctl::pairs();
  for (uint32_t i = 0; i < air::ctl::N_PAIRS; i++) out->lookup[i] = pair_active(tcfg, P[i]);
  auto rows = [&](int t) { return (uint64_t)1 << tcfg[t].log_n; };
  // Two seeded tables that a lookup ties together are ONE statement: the seeded sponge table asks for no more
  // permutations than the Keccak-f table holds in full, and the seeded Keccak-f table's first permutations are the
  // ones the sponge rows ask for (air::ctl, keccak_sponge -> keccak_f).  Tables given by the caller are taken as they are.
  const bool lookup_kf = out->lookup[L_SPONGE_KECCAK];
  // keccak_sponge -> logic: the XOR of every absorbed block with the rate is five operations of the logic table, whose
  // first rows are then derived from the sponge table's trace (five per covered sponge row; the caller's or seeded
  // operations follow them); the seeded sponge table absorbs no more blocks than the logic table can hold
  const bool lookup_sl = out->lookup[L_SPONGE_LOGIC];
  const uint32_t per_row = air::ctl::SPONGE_LOGIC_OPS;
  out->logic_covered = lookup_sl ? (uint32_t)std::min<uint64_t>(rows(T_KECCAK_SPONGE), rows(T_LOGIC) / per_row) : 0;
  out->sponge_row_limit = std::min<uint32_t>(lookup_kf ? (uint32_t)(rows(T_KECCAK) / TABLES[T_KECCAK].rows_per_item) : ~0u,
                                             lookup_sl ? out->logic_covered : ~0u);
  // byte_packing -> memory: the memory table that is not given by the caller is the log of the byte-packing table's
  // words (two operations per packing row); it must be tall enough to hold them
  const bool lookup_bm = out->lookup[L_PACKING_MEMORY];
  if (lookup_bm && given[T_BYTE_PACKING] && !given[T_MEMORY])
    return fail(BP_ERR_INVALID_INPUT, "byte-packing sequences are given but the memory log is not: the memory table is looked up by them "
                "(byte_packing -> memory) and cannot be drawn from the seed");
  // the mirror cases: a LOOKED table given by the caller while its looking table is drawn from the seed cannot be one
  // statement with it either (the seeded sponge rows ask for permutations of their own; the seeded packing rows move
  // words of their own) -- refused here, before seven table proofs are made and check_lookups blames the tables
  if (lookup_kf && given[T_KECCAK] && !given[T_KECCAK_SPONGE])
    return fail(BP_ERR_INVALID_INPUT, "Keccak-f permutations are given but the sponge rows are not: with both tables proven by their "
                "AIRs the sponge table looks the permutations up (keccak_sponge -> keccak_f); give the sponge rows too "
                "(bp_txn_witness.sponge_rows, bp_keccak256_sponge_rows) or clear the sponge table's AIR flag");
  if (lookup_bm && given[T_MEMORY] && !given[T_BYTE_PACKING])
    return fail(BP_ERR_INVALID_INPUT, "the memory log is given but the byte-packing sequences are not: the seeded byte-packing table "
                "looks up operations of its own (byte_packing -> memory); give the sequences too or clear one of the two AIR flags");
  if (lookup_bm && !given[T_MEMORY] && tcfg[T_MEMORY].log_n < tcfg[T_BYTE_PACKING].log_n + 1)
    return fail(BP_ERR_INVALID_INPUT, "the memory table (2^%u rows) cannot hold the operations of the byte-packing table (2^%u rows): "
                "two per row", tcfg[T_MEMORY].log_n, tcfg[T_BYTE_PACKING].log_n);
  // [five operations per covered sponge row][the caller's operations, or seeded ones]
  const uint64_t room = rows(T_LOGIC) - (uint64_t)per_row * out->logic_covered;
  if (lookup_sl && n_given[T_LOGIC] > room)
    return fail(BP_ERR_INVALID_INPUT, "the logic table (2^%u rows) holds the sponge table's %u XORs first: room for %llu operations, %zu given",
                tcfg[T_LOGIC].log_n, per_row * out->logic_covered, (unsigned long long)room, n_given[T_LOGIC]);
  return BP_OK;
}

uint32_t links_of(const StarkCfg tcfg[BP_NUM_TABLES], bp_set_link links[air::ctl::N_PAIRS], uint32_t pair[air::ctl::N_PAIRS]) {
  const air::ctl::Pair* P = air::ctl::pairs();
  uint32_t n = 0;
  for (uint32_t i = 0; i < air::ctl::N_PAIRS; i++) {
    const air::ctl::Pair& p = P[i];
    if (!pair_active(tcfg, p)) continue;
    bp_set_link& l = links[n] = bp_set_link{};
    l.n_looking = p.n_looking;
    for (uint32_t m = 0; m < p.n_looking; m++) l.looking[m] = bp_set_port{p.looking_table, p.looking_port + m};
    l.looked = bp_set_port{p.looked_table, p.looked_port};
    pair[n++] = i;
  }
  return n;
}

// The cross-table lookups of a transaction's table proofs, on the first-row openings (first_failing_link).  Shared by the
// prover (which refuses to go on with tables that do not form one statement: upstream's root circuit checks this
// in-circuit) and bp_verify_txn_table_proofs.
int check_lookups(const StarkCfg tcfg[BP_NUM_TABLES], const std::vector<uint64_t> proof[BP_NUM_TABLES]) {
  bp_set_link links[air::ctl::N_PAIRS];
  uint32_t pair[air::ctl::N_PAIRS], k, c;
  if (!first_failing_link(tcfg, proof, links, nullptr, links_of(tcfg, links, pair), &k, &c)) return BP_OK;
  const air::ctl::Pair& p = air::ctl::pairs()[pair[k]];
  return fail(BP_ERR_VERIFY, "cross-table lookup %s does not hold (challenge set %u): the %s table asks for tuples the %s table "
              "does not expose", p.name, c, TABLES[p.looking_table].name, TABLES[p.looked_table].name);
}

namespace {
// verify_proof(all_stark, all_proof, config) of upstream, on the CPU: every table proof against the shared transcript
// (trace caps and public values observed, four lookup challenges drawn, then table after table), and the cross-table
// lookups between the tables that are proven with their AIRs (air::ctl).  cfg supplies the STARK parameters only.
// expect (nullable): the statement the caller wants proven -- per table the AIR, height and width, and the public values --
// as parse_ir derives it from the transaction's IR.  Without it the header of the blob is the PROVER's claim.
int verify_table_proofs(const bp_config* cfg, const StarkCfg* expect, const uint64_t* expect_pv, const uint8_t* bytes, size_t len) {
  if (!cfg || !bytes) return fail(BP_ERR_INVALID_INPUT, "bp_verify_txn_table_proofs: null argument");
  if (len % 8 || len < (2 + BP_PV_WORDS + 4) * 8) return fail(BP_ERR_INVALID_INPUT, "table proofs: truncated");
  const uint64_t* W = reinterpret_cast<const uint64_t*>(bytes);
  const size_t n_words = len / 8;
  if (W[0] != TABLES_MAGIC || W[1] != BP_NUM_TABLES) return fail(BP_ERR_INVALID_INPUT, "table proofs: bad magic");
  const uint64_t* pv = W + 2;
  const uint64_t* ctl_in = pv + BP_PV_WORDS;
  for (size_t i = 0; i < BP_PV_WORDS + 4; i++) if (pv[i] >= gl::P) return fail(BP_ERR_VERIFY, "non-canonical public value or challenge");
  StarkCfg tcfg[BP_NUM_TABLES];
  std::vector<uint64_t> proof[BP_NUM_TABLES];
  size_t off = 2 + BP_PV_WORDS + 4;
  for (int t = 0; t < BP_NUM_TABLES; t++) {
    const char* name = TABLES[t].name;
    if (off + 4 > n_words) return fail(BP_ERR_INVALID_INPUT, "table proofs: truncated at table %s", name);
    const uint64_t air_id = W[off], log_n = W[off + 1], n_cols = W[off + 2], pw = W[off + 3];
    off += 4;
    if (air_id >= air::COUNT || log_n > 30 || n_cols > 65536) return fail(BP_ERR_INVALID_INPUT, "table proofs: bad header of table %s", name);
    if (air_id != air::SYNTHETIC && !table_has_air(t, (uint32_t)air_id))
      return fail(BP_ERR_VERIFY, "table %s is proven with AIR %llu, which is not that table's", name, (unsigned long long)air_id);
    tcfg[t] = table_cfg_of(*cfg, (uint32_t)log_n, (uint32_t)n_cols);
    tcfg[t].air_id = (uint32_t)air_id;
    if (expect && (expect[t].air_id != air_id || expect[t].log_n != log_n || expect[t].n_cols != n_cols))
      return fail(BP_ERR_VERIFY, "table %s is proven as AIR %llu, 2^%llu rows x %llu columns; the transaction's statement is AIR %u, 2^%u x %u "
                  "(a relabelled table would drop its constraints and its lookups)", name, (unsigned long long)air_id,
                  (unsigned long long)log_n, (unsigned long long)n_cols, expect[t].air_id, expect[t].log_n, expect[t].n_cols);
    int r = check_cfg(tcfg[t]);
    if (r) return r;
    if (pw != proof_layout(tcfg[t]).total || off + pw > n_words) return fail(BP_ERR_INVALID_INPUT, "table proofs: wrong length of table %s", name);
    proof[t].assign(W + off, W + off + pw);
    off += pw;
  }
  if (off != n_words) return fail(BP_ERR_INVALID_INPUT, "table proofs: trailing words");
  if (expect_pv && std::memcmp(pv, expect_pv, BP_PV_WORDS * 8) != 0)
    return fail(BP_ERR_VERIFY, "the public values of the table proofs are not those of the transaction's IR");
  Challenger ch;
  for (int t = 0; t < BP_NUM_TABLES; t++) {
    const ProofLayout L = proof_layout(tcfg[t]);
    ch.observe(proof[t].data() + L.trace_cap, L.cap_words);
  }
  ch.observe(pv, BP_PV_WORDS);
  Ctl ctl;
  for (int i = 0; i < 4; i++) {
    ctl.v[i] = ch.challenge();
    if (ctl.v[i] != ctl_in[i]) return fail(BP_ERR_VERIFY, "the lookup challenges do not follow from the trace commitments");
  }
  for (int t = 0; t < BP_NUM_TABLES; t++) {
    int r = stark_verify(tcfg[t], nullptr, ctl, ch, proof[t].data(), proof[t].size());
    if (r) {
      const std::string why = bp_last_error();
      return fail(r, "table %s: %s", TABLES[t].name, why.c_str());
    }
  }
  return check_lookups(tcfg, proof);
}
}  // namespace
}  // namespace txn
}  // namespace bpg

using namespace bpg;
using namespace bpg::txn;
extern "C" {

int bp_ir_encode(uint64_t block_number, uint64_t txn_number_before, uint64_t gas_used_before,
                 uint64_t gas_used_after, const uint64_t state_root_before[4], uint64_t seed,
                 const uint32_t table_log_n[BP_NUM_TABLES], const uint32_t table_width[BP_NUM_TABLES],
                 uint64_t o[BP_IR_WORDS]) {
  if (!state_root_before || !table_log_n || !table_width || !o) return fail(BP_ERR_INVALID_INPUT, "bp_ir_encode: null argument");
  o[0] = IR_MAGIC; o[1] = 1; o[2] = block_number; o[3] = txn_number_before; o[4] = gas_used_before; o[5] = gas_used_after;
  for (int i = 0; i < 4; i++) {
    if (state_root_before[i] >= gl::P) return fail(BP_ERR_INVALID_INPUT, "state root word is not a canonical field element");
    o[6 + i] = state_root_before[i];
  }
  o[10] = seed;
  for (int t = 0; t < BP_NUM_TABLES; t++) { o[11 + t] = table_log_n[t]; o[18 + t] = table_width[t]; }
  return BP_OK;
}
int bp_ir_encode_dummy(uint64_t block_number, uint64_t txn_number, uint64_t gas_used, const uint64_t state_root[4],
                       uint64_t seed, const uint32_t table_log_n[BP_NUM_TABLES], const uint32_t table_width[BP_NUM_TABLES],
                       uint64_t o[BP_IR_WORDS]) {
  int rc = bp_ir_encode(block_number, txn_number, gas_used, gas_used, state_root, seed, table_log_n, table_width, o);
  if (rc == BP_OK) o[1] = 2;
  return rc;
}

int bp_ir_set_keccak_air(uint64_t ir[BP_IR_WORDS], int on) { return ir_set_air(ir, T_KECCAK, 0, on); }
int bp_ir_set_logic_air(uint64_t ir[BP_IR_WORDS], int on) { return ir_set_air(ir, T_LOGIC, 0, on); }
int bp_ir_set_memory_air(uint64_t ir[BP_IR_WORDS], int on) { return ir_set_air(ir, T_MEMORY, 0, on); }
int bp_ir_set_arithmetic_air(uint64_t ir[BP_IR_WORDS], int on) { return ir_set_air(ir, T_ARITHMETIC, 0, on); }
int bp_ir_set_arithmetic_mul_air(uint64_t ir[BP_IR_WORDS], int on) { return ir_set_air(ir, T_ARITHMETIC, 1, on); }
int bp_ir_set_byte_packing_air(uint64_t ir[BP_IR_WORDS], int on) { return ir_set_air(ir, T_BYTE_PACKING, 0, on); }
int bp_ir_set_keccak_sponge_air(uint64_t ir[BP_IR_WORDS], int on) { return ir_set_air(ir, T_KECCAK_SPONGE, 0, on); }

int bp_verify_txn_table_proofs(const bp_config* cfg, const uint8_t* bytes, size_t len) try {
  return verify_table_proofs(cfg, nullptr, nullptr, bytes, len);
}
BPG_ABI_CATCH("bp_verify_txn_table_proofs")
// verify_proof(all_stark, ...) where the VERIFIER fixes the statement, as upstream's does: which AIR proves each table,
// the table shapes and the public values come from the transaction's IR, not from the blob.
int bp_verify_txn_table_proofs_for(const bp_config* cfg, const uint8_t* ir, size_t ir_len, const uint8_t* bytes, size_t len) try {
  if (!cfg || !ir) return fail(BP_ERR_INVALID_INPUT, "bp_verify_txn_table_proofs_for: null argument");
  if (ir_len != BP_IR_WORDS * 8) return fail(BP_ERR_INVALID_INPUT, "IR must be %d bytes", BP_IR_WORDS * 8);
  StarkCfg expect[BP_NUM_TABLES];
  std::vector<uint64_t> pv;
  int r = parse_ir(*cfg, reinterpret_cast<const uint64_t*>(ir), nullptr, expect, &pv);
  if (r) return r;
  return verify_table_proofs(cfg, expect, pv.data(), bytes, len);
}
BPG_ABI_CATCH("bp_verify_txn_table_proofs_for")

// What witness_of, parse_ir and plan_traces make of an IR and its witness data, without a device or a state: what the
// prover and the pre-flight decide before they touch the GPU, and their refusals.  data: nullable.
int bp_debug_txn_plan(const bp_config* cfg, const uint8_t* ir, size_t ir_len, const bp_txn_witness* data, bp_txn_plan* out) try {
  if (!cfg || !ir || !out) return fail(BP_ERR_INVALID_INPUT, "bp_debug_txn_plan: null argument");
  if (ir_len != BP_IR_WORDS * 8) return fail(BP_ERR_INVALID_INPUT, "IR must be %d bytes", BP_IR_WORDS * 8);
  std::memset(out, 0, sizeof(*out));
  TxnWitness wit;
  int r = witness_of(data, &wit);
  if (r) return r;
  StarkCfg tcfg[BP_NUM_TABLES];
  std::vector<uint64_t> pv;
  if ((r = parse_ir(*cfg, reinterpret_cast<const uint64_t*>(ir), &wit, tcfg, &pv))) return r;
  bool given[BP_NUM_TABLES];
  size_t n_given[BP_NUM_TABLES];
  for (int t = 0; t < BP_NUM_TABLES; t++) {
    given[t] = given_table(&wit, tcfg, t);
    n_given[t] = given[t] ? wit.n[t] : 0;
    out->table[t] = bp_txn_plan_table{tcfg[t].air_id, tcfg[t].n_cols, tcfg[t].log_n, given[t], TABLES[t].item_words,
                                      witness_capacity(t, (uint64_t)1 << tcfg[t].log_n)};
  }
  TracePlan plan;
  if ((r = plan_traces(tcfg, given, n_given, &plan))) return r;
  const air::ctl::Pair* P = air::ctl::pairs();
  for (uint32_t i = 0; i < air::ctl::N_PAIRS; i++)
    out->lookup[i] = bp_txn_plan_lookup{plan.lookup[i], P[i].looking_table, P[i].looking_air, P[i].looked_table, P[i].looked_air};
  out->logic_covered = plan.logic_covered;
  out->sponge_row_limit = plan.sponge_row_limit;
  return BP_OK;
}
BPG_ABI_CATCH("bp_debug_txn_plan")

}  // extern "C"
