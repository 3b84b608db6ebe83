// caller_table.hpp -- a caller's table, as every entry that takes one sees it (stark_api.cpp, table_set.cpp,
// air_check.cpp): an AIR and a shape, a device trace with a column stride, constant columns where the AIR reads some,
// four public inputs where it reads them.  What is refused about one, how one is committed on a transcript, and how a
// proving entry gets its worker and hands its proof out are each stated once, here and in caller_table.cpp.
#pragma once
#include <memory>
#include "prover.hpp"

namespace bpg {

inline StarkCfg to_cfg(const bp_stark_cfg& c, uint32_t air_id) {
  return StarkCfg{c.log_n, c.n_cols, c.n_const, c.deg_pow, c.rate_bits, c.cap_height, c.num_queries, c.pow_bits, c.arity_bits,
                  c.final_poly_bits, air_id};
}
inline bp_stark_cfg abi_cfg(const StarkCfg& c) {  // to_cfg's inverse (the id travels beside it)
  return bp_stark_cfg{c.log_n, c.n_cols, c.n_const, c.deg_pow, c.rate_bits, c.cap_height, c.num_queries, c.pow_bits, c.arity_bits,
                      c.final_poly_bits};
}

struct CallerTable {
  StarkCfg cfg;           // cfg.air_id: a built-in AIR or a registered program
  const uint64_t* trace;  // [n_cols] columns of 2^log_n words, `stride` words apart
  uint64_t stride;
  const uint64_t* consts;  // [n_const][2^log_n]; null when the AIR reads none
  const uint64_t* pub;     // four words, or null
  std::shared_ptr<const air::prog::Program> program;  // the registered program, if the id is one
  bool reads_public() const { return cfg.air_id == air::PLONK || (program && program->n_public); }
};
inline CallerTable caller_table(const StarkCfg& cfg, const uint64_t* trace, uint64_t stride, const uint64_t* consts, const uint64_t* pub) {
  return CallerTable{cfg, trace, stride, cfg.n_const ? consts : nullptr, pub, air::prog::find(cfg.air_id)};
}
// Everything an entry refuses about a table whose shape check_cfg has accepted, before any device call: a null trace, a
// stride shorter than the trace, constants missing where the AIR reads some, and the two refusals of check_public_inputs
// (the part of a table that belongs to a set's statement: public inputs missing where the AIR reads them, a public input
// that is no canonical word).  who: the entry; where: "" or "table %u: ".
int check_public_inputs(const char* who, const char* where, const CallerTable& t);
int check_caller_table(const char* who, const char* where, const CallerTable& t);

// The arena of one table proof: every oracle (values + coefficients + LDE) plus temporaries, and the trace once more
// when it has to be packed to stride 2^log_n.  An entry adds ARENA_SLACK once.
constexpr size_t ARENA_SLACK = 64u << 20;
size_t table_arena_bytes(const StarkCfg& c, bool packed);

// A worker (stream + arena of at least `bytes`) for the length of one call.  One worker is parked per device: a
// 2^20 x 2432 table needs a ~100 GB arena, and hipFree + hipMalloc of that much costs seconds -- several times the proof
// itself.  A call takes the parked worker if its arena is large enough (concurrent calls simply make their own), and
// parks its worker again (or frees it, when the slot is taken) on every way out, an exception included.
class WorkerLease {
 public:
  WorkerLease(int device, size_t bytes);
  ~WorkerLease();
  WorkerLease(const WorkerLease&) = delete;
  WorkerLease& operator=(const WorkerLease&) = delete;
  int rc() const { return rc_; }  // not BP_OK: there is no worker, and this is why
  Worker& operator*() const { return *w_; }

 private:
  Worker* w_ = nullptr;
  int rc_ = BP_OK;
};
void release_parked_workers();  // bp_release_cached_memory

// The table's commitments in transcript order: the constants (if any) and their cap observed, the trace -- packed to
// stride 2^log_n in the arena first when it is a column slice -- and its cap observed.  *d_values: the trace as committed.
int commit_caller_table(Worker& w, Challenger& ch, const CallerTable& t, Committed* consts, Committed* trace, const uint64_t** d_values);

// How a proving entry hands out its proof and ends.  emit: the words in a buffer for bp_free_buffer.  finish: nothing
// of the call is in flight when its worker is parked; a failed call keeps its own message; a call whose last wait fails
// hands out no buffer (*out null, *out_len 0).
int emit(const std::vector<uint64_t>& words, uint8_t** out, size_t* out_len);
int finish(Worker& w, int rc, uint8_t** out, size_t* out_len);

inline const bp_set_port& link_end(const bp_set_link& l, uint32_t m) { return m < l.n_looking ? l.looking[m] : l.looked; }  // m == n_looking: the looked port

// ---- tables tied port to port: a set's links, a transaction's active lookups (txn::links_of) -- table_set.cpp ----
// A link names its ends by (index into the tables, port); log_link[k]: link k is a link of log ports, whose identity is
// a sum (null: every link is a product link).  Neither function refuses anything about the statement: an unlinked port
// is legal for a transaction; what a public set refuses is check_set's.
//
// The identity on the first-row openings: for both challenge sets the product (a log link: the sum) of the looking
// ports' first-row values is the looked port's.  cfg[t], proof[t]: table t's shape and proof words.  True when a link
// fails: *link and *set name the first one and its challenge set.
bool first_failing_link(const StarkCfg* cfg, const std::vector<uint64_t>* proof, const bp_set_link* links, const bool* log_link,
                        uint32_t n_links, uint32_t* link, uint32_t* set);
// The pre-flight of tables and links: table[t] = bp_air_check_trace's answer for tables[t] (max_rows = max_viol = 8;
// a table without a trace is no member and is left alone), link[k] = the balance of link k on the device (set_check.hip)
// under one set of fresh challenges, as include/bpg.h defines bp_set_link_report.  Scratch: one hipMalloc of 64 bytes x
// the power of two >= twice the rows of the largest link's ends; BP_ERR_DEVICE under `who` when the device cannot give
// it.  Everything is checked; wording the first finding is the caller's.  Returns after `st` has finished.
int check_tables_and_links(const char* who, const CallerTable* tables, uint32_t n_tables, const bp_set_link* links, const bool* log_link,
                           uint32_t n_links, hipStream_t st, bp_set_table_report* table, bp_set_link_report* link);

}  // namespace bpg
