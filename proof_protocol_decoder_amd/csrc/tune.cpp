// tune.cpp -- the bp_tune_* entry points (bpg.h): each clamps its argument and stores it in bpg::Tune (tune.hpp).
#include "tune.hpp"
#include <cstdio>
#include "common.hpp"
#include "stark_kernels.hpp"

namespace bpg {
Tune& tune() {
  static Tune t;
  return t;
}
static_assert(MAX_BATCH == 8, "Tune::rec_batch's default is MAX_BATCH");
static_assert(MAX_LOCKSTEP >= 3 * MAX_BATCH, "a group of three transactions fills one lock-step batch per level");
}  // namespace bpg

// every knob, in the order bp_debug_tune_state reports them
#define BPG_KNOBS(X)                                                                                            \
  X(quad_threshold) X(assume_loaded) X(merkle_fused) X(merkle_wide) X(poseidon_mx) X(poseidon_mx_sets)          \
  X(poseidon_grouped) X(ntt_mx) X(ntt_split) X(k5_spread) X(host_wait) X(host_poseidon) X(rec_batch)            \
  X(witness_threads) X(side_lanes)

extern "C" {

void bp_tune_quad_threshold(uint64_t n_perms) { bpg::tune().quad_threshold.store(n_perms); }
void bp_tune_assume_loaded(int mode) { bpg::tune().assume_loaded.store(mode < 0 ? -1 : (mode != 0)); }
void bp_tune_merkle_fused(int mode) { bpg::tune().merkle_fused.store(mode < 0 ? -1 : (mode != 0)); }
void bp_tune_merkle_wide(int log2_parents) { bpg::tune().merkle_wide.store(log2_parents < 8 || log2_parents > 24 ? 0 : log2_parents); }
void bp_tune_poseidon_mx(int on) { bpg::tune().poseidon_mx.store(on != 0); }
void bp_tune_poseidon_mx_sets(int sets) { bpg::tune().poseidon_mx_sets.store(sets == 1 || sets == 2 || sets == 4 ? sets : 0); }
void bp_tune_poseidon_grouped(int on) { bpg::tune().poseidon_grouped.store(on != 0); }
void bp_tune_ntt_mx(int mode) { bpg::tune().ntt_mx.store(mode < 0 || mode > 3 ? 3 : mode); }
void bp_tune_ntt_split(int mode) { bpg::tune().ntt_split.store(mode == 1 || mode == 2 ? mode : 0); }
void bp_tune_k5_spread(int on) { bpg::tune().k5_spread.store(on != 0); }
void bp_tune_host_wait(int mode) { bpg::tune().host_wait.store(mode < 0 || mode > 2 ? 0 : mode); }
void bp_tune_host_poseidon(int mode) { bpg::tune().host_poseidon.store(mode == 1 ? 1 : 0); }
void bp_tune_rec_batch(int n) { bpg::tune().rec_batch.store(n < 1 ? 1 : (n > (int)bpg::MAX_BATCH ? (int)bpg::MAX_BATCH : n)); }
void bp_tune_witness_threads(int n) { bpg::tune().witness_threads.store(n < 1 ? 1 : (n > 16 ? 16 : n)); }
void bp_tune_side_lanes(int n) { bpg::tune().side_lanes.store(n < 0 ? 0 : n); }
// A switch between two schedules of the same proofs, not one of the kernel knobs that bp_debug_tune_state lists (its
// lines are a fixed set); bp_tune_reset puts it back like the others.
void bp_tune_rec_riders(int on) { bpg::tune().rec_riders.store(on != 0); }
// Another schedule of the same proofs (tune.hpp): like rec_riders outside bp_debug_tune_state's fixed lines.
void bp_tune_txn_group(int n) { bpg::tune().txn_group.store(n < 1 ? 0 : (n > (int)bpg::MAX_BATCH ? (int)bpg::MAX_BATCH : n)); }
// Another schedule of the same proofs (tune.hpp): 0 = a group's recursion levels as lock-step batches over the group,
// 1 = one transaction's recursion at a time.
void bp_tune_rec_group(int mode) { bpg::tune().rec_group.store(mode == 1 ? 1 : 0); }
// The switch point between two forms of one kernel (range_mult.hip); like rec_riders outside bp_debug_tune_state's fixed
// lines.  Out of range = the default.
void bp_tune_range_lds_log(int log_range) {
  bpg::tune().range_lds_log.store(log_range < 1 || log_range > 14 ? bpg::Tune().range_lds_log.load() : log_range);
}

void bp_tune_reset(void) {
  const bpg::Tune defaults;
  bpg::Tune& t = bpg::tune();
#define X(k) t.k.store(defaults.k.load());
  BPG_KNOBS(X)
#undef X
  t.rec_riders.store(defaults.rec_riders.load());
  t.txn_group.store(defaults.txn_group.load());
  t.rec_group.store(defaults.rec_group.load());
  t.range_lds_log.store(defaults.range_lds_log.load());
}

int bp_debug_tune_state(char* buf, size_t cap) {
  if (!buf || !cap) return bpg::fail(BP_ERR_INVALID_INPUT, "bp_debug_tune_state: no buffer");
  const bpg::Tune& t = bpg::tune();
  size_t n = 0;
#define X(k)                                                                                   \
  if (n < cap) {                                                                               \
    const int w = std::snprintf(buf + n, cap - n, #k "=%lld\n", (long long)t.k.load());         \
    n += w > 0 ? (size_t)w : 0;                                                                \
  }
  BPG_KNOBS(X)
#undef X
  if (n >= cap) return bpg::fail(BP_ERR_INVALID_INPUT, "bp_debug_tune_state: buffer of %zu bytes is too small", cap);
  return BP_OK;
}

}  // extern "C"
