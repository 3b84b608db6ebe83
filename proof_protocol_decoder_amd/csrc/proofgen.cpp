// proofgen.cpp -- L1 of the C ABI: prover/verifier state and the txn / agg / block entry points,
// mirroring plonky_block_proof_gen/src/{prover_state.rs, proof_gen.rs, verifier_state.rs,
// proof_types.rs}.  What each call computes is the synthetic workload of SURVEY.md section 8(d)
// (DESIGN.md section 5); the control flow, ownership, threading and error behaviour follow the
// reference (see include/bpg.h).
#include <algorithm>
#include <array>
#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <string>
#include <system_error>
#include <thread>
#include <deque>
#include <functional>
#include <set>
#include "caller_table.hpp"
#include "mpt.hpp"
#include "prover.hpp"
#include "rec_pool.hpp"
#include "tune.hpp"
#include "txn_tables.hpp"
#include "worker_table.hpp"

using namespace bpg;
using namespace bpg::txn;
extern "C" int bp_use_blocking_sync(int device);
extern "C" int bp_host_wait_mode(int device);

namespace {

constexpr uint64_t PROOF_BOX_MAGIC = 0x464F4F5250475042ULL;  // "BPGPROOF"
constexpr uint32_t CIRCUIT_ROOT = 7, CIRCUIT_AGG = 8, CIRCUIT_BLOCK = 9;
constexpr uint32_t AGG_PATH_PI0 = 10, BLOCK_PATH_PI0 = 9;  // where the children's (leaf digest, cap entry) words sit in the list
constexpr uint32_t CHAIN_PATH_PI0 = 6, ROOT_PATH_PI0 = 4 * BP_NUM_TABLES;  // ... of a chain circuit's one child, of the root circuit's seven
constexpr uint32_t SHRINK_SEED_DEGREE = 255;  // circuit_seed(table, 255): the table's shrink circuit (levels >= 1 of its chain)
constexpr size_t BOX_HDR = 4;

uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}
uint64_t circuit_seed(uint32_t table_or_kind, uint32_t degree) {
  return splitmix64(0xC12C0175EEDULL + ((uint64_t)table_or_kind << 8) + degree);
}

struct Circuit {  // one preprocessed recursion circuit: constants commitment + its digest
  uint64_t* d_const_values = nullptr;
  Committed consts;
  uint64_t digest[4];
  air::plonk::Layout lay{};  // AIR 8: the list the circuit hashes and the Merkle paths it walks
};
// (PathWitness, one Merkle path a recursion circuit walks: rec_pool.hpp -- a job carries them)
struct LightCircuit {
  std::vector<uint64_t> cap;
  uint64_t digest[4];
};

}  // namespace

struct bp_state {
  bp_config cfg;
  StarkCfg rec_cfg;
  Worker builder;                       // owns the persistent (preprocessed) device memory
  std::vector<Circuit> table_circuits;  // [table][degree - lo] flattened: level 0 of a table's chain (its child is the table's STARK proof)
  Circuit shrink_circuits[BP_NUM_TABLES];  // levels >= 1 of a table's chain (their child is a recursion-shaped proof)
  uint32_t table_offset[BP_NUM_TABLES];
  Circuit special[3];                   // root, agg, block
  // worker pool: `&ProverState` is shared by many threads in the reference (proof_gen.rs:40)
  mutable std::mutex mu;
  mutable std::condition_variable cv;
  mutable std::vector<std::unique_ptr<Worker>> workers;
  // The workers' arenas are slices of a few large device allocations (one, where the device grants it): the slices of a
  // slab lie one behind the other, stride slice_stride, so a run of adjacent idle workers is one contiguous piece of
  // memory (ProverLease).  table: who is idle, who is whose neighbour (worker_table.hpp); under mu.
  std::vector<void*> slabs;
  size_t slice_stride = 0;
  mutable WorkerTable table;
  uint32_t auto_txn_group = 1;  // Tune::txn_group = 0: what this state's queue count asks for (bp_state_build)
  // Keccak-256 of every proof container this state has produced (bounded): aggregation verifies its children on the
  // host (verify_child), which costs 10 ms of CPU per recursion-shaped proof against 5 ms of GPU to make one -- a child
  // that this very state has just produced, byte for byte, is recognised instead of being verified again
  mutable std::mutex seen_mu;
  mutable std::set<mpt::H256> seen;
  mutable std::deque<mpt::H256> seen_order;
  std::string warnings;  // bp_state_warnings: what bp_state_build found about the environment it runs in
};
struct bp_verifier_state {
  StarkCfg rec_cfg;
  LightCircuit special[3];
};

namespace {

// The prover(s) a call works on.  want == 1 (every call but a group of transactions): one worker by take_one's rule --
// an idle worker with no idle neighbour first, else the one released last -- which spares the runs for groups.
// want > 1 (the transactions a prover takes at a time, Tune::txn_group): a RUN of workers whose arenas are neighbours,
// up to `want` adjacent idle workers, all or nothing under bp_state::mu -- the longest adjacent run there is when `want`
// are not to be had, never a wait for adjacency.  Either way the lease blocks only while no worker is idle and holds
// nothing while it waits.  The first worker of the run leads: its stream, its mailbox, and for the time of the lease an
// arena that spans the run's slices.  The others lend their pinned buffers (witness staging); their streams stay idle.
// A worker that kept something in its arena across leases (none does: every lease releases to the mark it found, which
// is 0) would end the run in front of it: the spanning view covers clean slices only.
struct ProverLease {
  const bp_state* s;
  std::vector<Worker*> ws;  // ws[0] leads
  Worker* w;                // ws[0]
  uint32_t first = 0;
  size_t mark = 0, own_cap = 0;
  explicit ProverLease(const bp_state* st, uint32_t want = 1) : s(st) {
    std::unique_lock<std::mutex> lk(s->mu);
    s->cv.wait(lk, [&] { return s->table.any_idle(); });
    uint32_t n = 1;
    if (want > 1) {
      n = s->table.take_run(want, &first);
      uint32_t clean = 1;
      while (clean < n && s->workers[first + clean]->arena.mark() == 0) clean++;
      for (uint32_t k = clean; k < n; k++) s->table.give(first + k);
      n = clean;
    } else {
      first = (uint32_t)s->table.take_one();
    }
    for (uint32_t k = 0; k < n; k++) ws.push_back(s->workers[first + k].get());
    w = ws[0];
    mark = w->arena.mark();
    own_cap = w->arena.capacity();
    w->arena.span((size_t)(n - 1) * s->slice_stride + own_cap);
    prover_active((int)n);  // a group counts as the transactions it proves: the load-dependent choices see today's load
  }
  uint32_t size() const { return (uint32_t)ws.size(); }
  ~ProverLease() {
    prover_active(-(int)ws.size());
    (void)hipStreamSynchronize(w->stream);
    w->arena.release(mark);
    w->arena.span(own_cap);
    w->abort_flag = nullptr;
    w->abort_flag_u8 = nullptr;
    std::lock_guard<std::mutex> lk(s->mu);
    for (uint32_t k = 0; k < ws.size(); k++) s->table.give(first + k);
    s->cv.notify_all();
  }
};

// An idle worker borrowed as a LANE -- its stream and its cap mailbox, nothing else -- by a prover that finds itself
// ALONE on the device (a lone transaction, the last one of a shard): work that does not depend on each other (the seven
// trace commitments of a transaction) then overlaps instead of running one medium launch after the other.  Never waits
// for a worker, is not counted as a prover.  (Streams of their own for this were measured and dropped: three more streams
// in the process cost the loaded 256-txn block 2.6 % whether they were used or not -- 24 streams instead of 21, the same
// step the stream sweep shows between 20 and 24 prover streams.)
struct SideLane {
  const bp_state* s;
  Worker* w;
  uint32_t index;
  static std::unique_ptr<SideLane> try_acquire(const bp_state* st) {
    std::lock_guard<std::mutex> lk(st->mu);
    const int i = st->table.take_one();
    if (i < 0) return nullptr;
    return std::unique_ptr<SideLane>(new SideLane{st, st->workers[i].get(), (uint32_t)i});
  }
  ~SideLane() {
    (void)hipStreamSynchronize(w->stream);  // nothing of ours is left on the lane when its owner gets it back
    std::lock_guard<std::mutex> lk(s->mu);
    s->table.give(index);
    s->cv.notify_all();
  }
};

StarkCfg rec_cfg_of(const bp_config& c) {
  return StarkCfg{c.rec_log_n, c.rec_n_cols, c.rec_n_const, 3, c.rec_rate_bits, c.stark_cap_height,
                  c.rec_num_queries, c.rec_pow_bits, c.arity_bits, c.final_poly_bits, c.rec_air_id};
}
// lay (AIR 8): the public-input list the circuit's hash rows absorb -- 6 words for a table's chain circuits (digest,
// table, depth), 7 x 4 + 13 for the root circuit, 10 + 2 x 8 + 13 / 9 + 8 + 13 for the aggregation / block circuit -- and
// the Merkle paths it walks: one per child proof of the aggregation circuit, the aggregation child's of the block circuit
int build_circuit(Worker& w, const StarkCfg& rc, uint64_t seed, const air::plonk::Layout& lay, Circuit* out) {
  const uint64_t N = (uint64_t)1 << rc.log_n;
  out->lay = lay;
  out->d_const_values = w.arena.alloc_words((size_t)rc.n_const * N);
  if (!out->d_const_values) return fail(BP_ERR_DEVICE, "state arena exhausted");
  int rc2 = rc.air_id == air::PLONK ? launch_plonk_constants(out->d_const_values, rc.log_n, seed, lay, w.stream)
                                    : launch_synth_constants(out->d_const_values, rc.log_n, rc.n_const, seed, w.stream);
  if (rc2) return rc2;
  if ((rc2 = commit(w, out->d_const_values, rc.n_const, rc.log_n, rc.rate_bits, rc.cap_height, false, &out->consts)))
    return rc2;
  hash_no_pad_host(out->consts.cap.data(), out->consts.cap.size(), out->digest);
  return BP_OK;
}

struct Box {  // parsed proof container
  uint64_t kind, n_pi, circuit;
  const uint64_t *pi, *pv, *stark;
  size_t stark_words;
};
int parse_box(const uint8_t* bytes, size_t len, const StarkCfg& rc, Box* b) {
  if (!bytes || len % 8 || len < (BOX_HDR + BP_PV_WORDS) * 8) return fail(BP_ERR_INVALID_INPUT, "proof: truncated");
  const uint64_t* wds = reinterpret_cast<const uint64_t*>(bytes);
  if (wds[0] != PROOF_BOX_MAGIC) return fail(BP_ERR_INVALID_INPUT, "proof: bad magic");
  b->kind = wds[1]; b->n_pi = wds[2]; b->circuit = wds[3];
  if (b->kind > 2 || b->n_pi < BP_PV_WORDS || b->n_pi > air::plonk::MAX_PI) return fail(BP_ERR_INVALID_INPUT, "proof: bad header");
  const size_t sw = proof_layout(rc).total;
  if (len / 8 != BOX_HDR + b->n_pi + sw) return fail(BP_ERR_INVALID_INPUT, "proof: wrong length for this circuit");
  b->pi = wds + BOX_HDR;
  b->pv = b->pi + b->n_pi - BP_PV_WORDS;
  b->stark = b->pi + b->n_pi;
  b->stark_words = sw;
  return BP_OK;
}
int emit_box(uint64_t kind, uint64_t circuit, const std::vector<uint64_t>& pi, const std::vector<uint64_t>& stark,
             uint8_t** out, size_t* out_len) {
  const size_t words = BOX_HDR + pi.size() + stark.size();
  uint64_t* o = static_cast<uint64_t*>(std::malloc(words * 8));
  if (!o) return fail(BP_ERR_DEVICE, "host allocation failed");
  o[0] = PROOF_BOX_MAGIC; o[1] = kind; o[2] = pi.size(); o[3] = circuit;
  std::memcpy(o + BOX_HDR, pi.data(), pi.size() * 8);
  std::memcpy(o + BOX_HDR + pi.size(), stark.data(), stark.size() * 8);
  *out = reinterpret_cast<uint8_t*>(o);
  *out_len = words * 8;
  return BP_OK;
}

// proofs of shape rc one lock-step batch holds: MAX_BATCH, Tune::rec_batch, and the query launches' index limit
uint32_t batch_cap(const StarkCfg& rc) {
  return std::min<uint32_t>(std::min<uint32_t>(MAX_BATCH, std::max<uint32_t>(1, tune().rec_batch.load(std::memory_order_relaxed))),
                            std::max<uint32_t>(1, MAX_BATCH_QUERIES / std::max<uint32_t>(1, rc.num_queries)));
}
// What the mailbox holds of a lock-step batch of shape c: every proof's caps, its openings, its last FRI layer (the
// query openings fall back to the arena by themselves).
size_t mailbox_cap(const StarkCfg& c, size_t pinned_words) {
  const ProofLayout L = proof_layout(c);
  const size_t open_words = ((size_t)c.n_const + c.n_cols + 2 * (size_t)L.n_aux + L.n_quot) * 4;
  const size_t last_layer = (size_t)2 * ((size_t)L.final_len << c.rate_bits);
  const size_t per_proof = std::max(std::max(open_words, last_layer), L.cap_words);
  return pinned_words / std::max<size_t>(1, per_proof);
}
// ... and one sub-batch of rec_prove_batch for a caller that brings the levels of n_txn transactions: n_txn times what
// one transaction's level takes (batch_cap: the arena of a transaction is sized for that, and a group holds n_txn of
// them), within what a launch accepts -- MAX_LOCKSTEP blocks, MAX_BATCH_QUERIES indices -- and the mailbox holds.
uint32_t lockstep_cap(const StarkCfg& rc, size_t pinned_words, uint32_t n_txn) {
  size_t cap = std::min<size_t>(MAX_LOCKSTEP, MAX_BATCH_QUERIES / std::max<uint32_t>(1, rc.num_queries));
  cap = std::min(cap, mailbox_cap(rc, pinned_words));
  cap = std::min(cap, (size_t)batch_cap(rc) * std::max<uint32_t>(1, n_txn));
  return (uint32_t)std::max<size_t>(1, cap);
}
// rec_prove_batch's sub-batches by size (bp_debug_rec_batch_histogram)
std::atomic<uint64_t>* rec_batch_sizes() {
  static std::atomic<uint64_t> n[MAX_LOCKSTEP + 1];
  return n;
}
// Recursion-shaped proofs; transcript of each = circuit digest, hash of the public inputs, trace cap.  `n` proofs of
// the state's one recursion shape are proved in lock-step, up to Tune::rec_batch at a time (stark_prove_batch: every
// launch and every host wait is shared; circuits, public inputs and transcripts are each proof's own).
// paths (nullable): per proof the witness of the Merkle paths its circuit walks (Circuit::lay.n_paths of them)
// first_leaf (nullable, 4 words per proof): the digest of the trace leaf each proof's first query opens
// n_txn: the transactions whose levels the caller brings (a group's recursion: lockstep_cap) -- a batch that would pass
// a limit is split, never failed
int rec_prove_batch(Worker& w, const StarkCfg& rc, uint32_t n, const Circuit* const* circ, const std::vector<uint64_t>* pi,
                    std::vector<uint64_t>* proofs, const std::vector<PathWitness>* paths = nullptr, uint64_t* first_leaf = nullptr,
                    uint32_t n_txn = 1) {
  const uint32_t cap = lockstep_cap(rc, w.pinned_words, n_txn);
  const uint64_t N = (uint64_t)1 << rc.log_n;
  for (uint32_t first = 0; first < n; first += cap) {
    const uint32_t B = std::min(cap, n - first);
    rec_batch_sizes()[B].fetch_add(1, std::memory_order_relaxed);
    const size_t mark = w.arena.mark();
    uint64_t* d_trace = w.arena.alloc_words((size_t)B * rc.n_cols * N);
    if (!d_trace) return fail(BP_ERR_DEVICE, "device arena exhausted (%zu MiB)", w.arena.capacity() >> 20);
    Challenger ch[MAX_LOCKSTEP];
    SynthTraceArgs sa[MAX_LOCKSTEP];
    PlonkTraceArgs pa[MAX_LOCKSTEP];
    Ctl ctl[MAX_LOCKSTEP];
    const uint64_t* d_tv[MAX_LOCKSTEP];
    const Committed* consts[MAX_LOCKSTEP];
    // The witness of every proof's Poseidon rows is made on the host (prover.hpp): per proof the sponge over its list, per
    // path the Merkle rows and -- where the circuit hashes its leaves -- the sponge over the opened row.  The pieces are
    // independent; a prover that is alone on the device (a lone transaction: this is its critical path) makes them on up
    // to seven threads.
    uint64_t pi_hashes[MAX_LOCKSTEP][4];
    struct Job {
      uint32_t b, kind, p;  // kind 0: the list's rows, 1: path p's Merkle rows, 2: path p's leaf rows
    };
    std::vector<Job> jobs;
    for (uint32_t b = 0; b < B; b++) {
      const Circuit& c = *circ[first + b];
      const size_t n_pi = pi[first + b].size();
      if (rc.air_id != air::PLONK) {
        hash_no_pad_host(pi[first + b].data(), n_pi, pi_hashes[b]);
        continue;
      }
      if (n_pi < 1 || n_pi > air::plonk::MAX_PI) return fail(BP_ERR_INVALID_INPUT, "a recursion circuit hashes 1..%u public inputs: got %zu", air::plonk::MAX_PI, n_pi);
      if (n_pi != c.lay.pi_len) return fail(BP_ERR_INVALID_INPUT, "this circuit hashes a list of %u public inputs: got %zu", c.lay.pi_len, n_pi);
      jobs.push_back(Job{b, 0, 0});
      if (c.lay.n_paths) {
        if (!paths || paths[first + b].size() != c.lay.n_paths) return fail(BP_ERR_INVALID_INPUT, "this circuit walks %u Merkle paths: their witness is missing", c.lay.n_paths);
        for (uint32_t p = 0; p < c.lay.n_paths; p++) {
          const PathWitness& pw = paths[first + b][p];
          if (pw.siblings.size() != 4 * (size_t)c.lay.depth) return fail(BP_ERR_INVALID_INPUT, "Merkle path %u: %zu sibling words for %u levels", p, pw.siblings.size(), c.lay.depth);
          if (c.lay.leaf_len && pw.leaf_row.size() != c.lay.leaf_len) return fail(BP_ERR_INVALID_INPUT, "Merkle path %u: the circuit hashes a leaf of %u words, %zu given", p, c.lay.leaf_len, pw.leaf_row.size());
          jobs.push_back(Job{b, 1, p});
          if (c.lay.leaf_len) jobs.push_back(Job{b, 2, p});
        }
      }
    }
    auto run_job = [&](const Job& j) {
      const Circuit& c = *circ[first + j.b];
      uint64_t* hr = w.hash_rows + (size_t)j.b * HASH_ROWS_WORDS;
      std::vector<uint64_t> rows;
      if (j.kind == 0) {  // the hash of the public-input list, with the witness of the circuit's own computation of it
        poseidon_hash_rows(pi[first + j.b].data(), pi[first + j.b].size(), &rows, pi_hashes[j.b]);
        std::memcpy(hr, rows.data(), rows.size() * 8);
      } else if (j.kind == 1) {  // a child's Merkle path, walked the way the circuit's rows walk it
        const PathWitness& pw = paths[first + j.b][j.p];
        uint64_t root[4];  // (not compared with the list's cap entry here: the copy constraints do that, and the verifier)
        poseidon_merkle_rows(&pi[first + j.b][c.lay.path_pi0 + 8 * j.p], pw.index, pw.siblings.data(), c.lay.depth,
                             hr + (size_t)(air::plonk::HASH_ROWS_MAX + j.p * c.lay.depth) * air::plonk::H_WIRES, root);
      } else {  // the sponge over the opened row that the leaf digest is the hash of
        const PathWitness& pw = paths[first + j.b][j.p];
        uint64_t leaf_digest[4];
        poseidon_hash_rows(pw.leaf_row.data(), c.lay.leaf_len, &rows, leaf_digest);
        std::memcpy(hr + (size_t)(air::plonk::HASH_ROWS_MAX + air::plonk::merkle_rows(c.lay) + j.p * air::plonk::hash_rows(c.lay.leaf_len)) * air::plonk::H_WIRES,
                    rows.data(), rows.size() * 8);
      }
    };
    {
      const uint32_t max_threads = (uint32_t)std::max(1, tune().witness_threads.load(std::memory_order_relaxed));
      const uint32_t n_threads = (provers_active() <= 1 && jobs.size() >= 4) ? (uint32_t)std::min<size_t>(max_threads, jobs.size()) : 1;
      std::atomic<size_t> next{0};
      std::atomic<bool> oom{false};
      auto drain = [&] {
        try {
          for (size_t k; (k = next.fetch_add(1)) < jobs.size();) run_job(jobs[k]);
        } catch (...) {
          oom.store(true);
        }
      };
      std::vector<std::thread> pool;
      struct Join {
        std::vector<std::thread>& p;
        ~Join() { for (auto& t : p) if (t.joinable()) t.join(); }
      } join{pool};
      try {
        for (uint32_t t = 1; t < n_threads; t++) pool.emplace_back(drain);
      } catch (const std::system_error&) {  // no thread to be had: this one does the rest
      }
      drain();
      for (auto& t : pool) t.join();
      pool.clear();
      if (oom.load()) return fail(BP_ERR_DEVICE, "out of memory while making the witness of the Poseidon rows");
    }
    for (uint32_t b = 0; b < B; b++) {
      const Circuit& c = *circ[first + b];
      const uint64_t* pi_hash = pi_hashes[b];
      const size_t n_pi = pi[first + b].size();
      ch[b].observe(c.digest, 4);
      ch[b].observe(pi_hash, 4);
      d_tv[b] = d_trace + (size_t)b * rc.n_cols * N;
      sa[b] = SynthTraceArgs{d_trace + (size_t)b * rc.n_cols * N, c.d_const_values, pi_hash[0]};
      pa[b] = PlonkTraceArgs{d_trace + (size_t)b * rc.n_cols * N, c.d_const_values, pi_hash[0], {pi_hash[0], pi_hash[1], pi_hash[2], pi_hash[3]},
                             w.hash_rows_dev + (size_t)b * HASH_ROWS_WORDS, (uint32_t)((n_pi + 7) / 8),
                             air::plonk::merkle_rows(c.lay) + air::plonk::leaf_rows(c.lay), air::plonk::arith_row0(c.lay)};
      if (rc.air_id == air::PLONK) std::memcpy(ctl[b].pub, pi_hash, 32);  // bound to the circuit's first row
      consts[b] = &c.consts;
    }
    int r = rc.air_id == air::PLONK ? launch_plonk_trace(pa, B, rc.log_n, w.stream)
                                    : launch_synth_trace(sa, B, rc.log_n, rc.n_cols, rc.n_const, rc.deg_pow, w.stream);
    if (r) return r;
    Committed trace[MAX_LOCKSTEP];
    if ((r = commit_batch(w, d_trace, rc.n_cols, B, rc.log_n, rc.rate_bits, rc.cap_height, false, trace))) return r;
    for (uint32_t b = 0; b < B; b++) {
      ch[b].observe(trace[b].cap.data(), trace[b].cap.size());
      for (int i = 0; i < 4; i++) ctl[b].v[i] = ch[b].challenge();
    }
    r = stark_prove_batch(w, rc, B, consts, trace, d_tv, ctl, ch, proofs + first, first_leaf ? first_leaf + 4 * first : nullptr);
    w.arena.release(mark);
    if (r) return r;
  }
  return BP_OK;
}
int rec_prove(Worker& w, const StarkCfg& rc, const Circuit& circ, const std::vector<uint64_t>& pi,
              std::vector<uint64_t>& proof, const std::vector<PathWitness>* paths = nullptr) {
  const Circuit* c = &circ;
  return rec_prove_batch(w, rc, 1, &c, &pi, &proof, paths);
}
// What the aggregation / block circuit walks for a child: the Merkle path of the child's FIRST query into its trace
// oracle.  leaf = the digest of the opened trace row, cap_entry = the entry of the child's trace cap the path ends in
// (both become words of the parent's public-input list), pw = position and siblings.  `child` has been parsed
// (parse_box: its length is the layout's).
// known_leaf (nullable): the leaf digest as the prover's device gave it (stark_prove's first_trace_leaf) -- a child made
// elsewhere has its opened row hashed here.
void first_query_trace_path(const StarkCfg& c, const uint64_t* child, uint64_t leaf[4], uint64_t cap_entry[4], PathWitness* pw,
                            const uint64_t* known_leaf = nullptr) {
  const ProofLayout L = proof_layout(c);
  const uint64_t* w = child + L.queries;
  const uint64_t x = *w++;
  if (c.n_const) w += c.n_const + (size_t)L.depth0 * 4;
  pw->leaf_row.assign(w, w + c.n_cols);
  if (known_leaf) {
    std::memcpy(leaf, known_leaf, 32);
  } else if (c.n_cols <= 4) {  // Hasher::hash_or_noop
    std::memset(leaf, 0, 32);
    std::memcpy(leaf, w, c.n_cols * 8);
  } else {
    hash_no_pad_host(w, c.n_cols, leaf);
  }
  w += c.n_cols;
  pw->index = x & (((uint64_t)1 << L.depth0) - 1);
  pw->siblings.assign(w, w + 4 * (size_t)L.depth0);
  const uint64_t top = (x >> L.depth0) & (((uint64_t)1 << c.cap_height) - 1);
  std::memcpy(cap_entry, child + L.trace_cap + 4 * top, 32);
}
// the length of the public-input list each kind of container carries (what its circuit hashes in its thirteen rows at most)
uint32_t box_pi_len(uint64_t kind) {
  return kind == 0 ? ROOT_PATH_PI0 + 8 * BP_NUM_TABLES + BP_PV_WORDS : kind == 1 ? AGG_PATH_PI0 + 16 + BP_PV_WORDS : BLOCK_PATH_PI0 + 8 + BP_PV_WORDS;
}
int rec_verify(const StarkCfg& rc, const LightCircuit& circ, const Box& b) {
  if (b.n_pi != box_pi_len(b.kind))
    return fail(BP_ERR_VERIFY, "a proof of kind %llu carries %u public inputs, this one %llu", (unsigned long long)b.kind, box_pi_len(b.kind),
                (unsigned long long)b.n_pi);
  uint64_t pi_hash[4];
  hash_no_pad_host(b.pi, b.n_pi, pi_hash);
  Challenger ch;
  ch.observe(circ.digest, 4);
  ch.observe(pi_hash, 4);
  const ProofLayout L = proof_layout(rc);
  ch.observe(b.stark + L.trace_cap, L.cap_words);
  Ctl ctl;
  for (int i = 0; i < 4; i++) ctl.v[i] = ch.challenge();
  if (rc.air_id == air::PLONK) std::memcpy(ctl.pub, pi_hash, sizeof(pi_hash));
  return stark_verify(rc, circ.cap.data(), ctl, ch, b.stark, b.stark_words);
}

// What the real aggregation / block circuits do in-circuit (prove_aggregation / prove_block verify their
// children, proof_gen.rs:66-75, 97-103) is done on the host here: a child container is accepted only if
// it was made by the circuit its kind names, its public inputs are canonical and its proof verifies
// against this state's preprocessed circuit.
constexpr size_t SEEN_MAX = 8192;
void remember_proof(const bp_state* s, const uint8_t* bytes, size_t len) {
  const mpt::H256 h = mpt::keccak256(bytes, len);
  std::lock_guard<std::mutex> lk(s->seen_mu);
  if (!s->seen.insert(h).second) return;
  s->seen_order.push_back(h);
  if (s->seen_order.size() > SEEN_MAX) {
    s->seen.erase(s->seen_order.front());
    s->seen_order.pop_front();
  }
}
bool produced_here(const bp_state* s, const uint8_t* bytes, size_t len) {
  const mpt::H256 h = mpt::keccak256(bytes, len);
  std::lock_guard<std::mutex> lk(s->seen_mu);
  return s->seen.count(h) != 0;
}

int verify_foreign(const bp_state* s, const Box& b, const char* what) {
  if (b.circuit != CIRCUIT_ROOT + b.kind)
    return fail(BP_ERR_VERIFY, "%s was made by circuit %llu, expected %u", what, (unsigned long long)b.circuit,
                CIRCUIT_ROOT + (uint32_t)b.kind);
  for (size_t i = 0; i < b.n_pi; i++)
    if (b.pi[i] >= gl::P) return fail(BP_ERR_VERIFY, "%s: non-canonical public input", what);
  LightCircuit lc;
  lc.cap = s->special[b.kind].consts.cap;
  std::memcpy(lc.digest, s->special[b.kind].digest, 32);
  int r = rec_verify(s->rec_cfg, lc, b);
  if (r) {
    const std::string why = bp_last_error();
    return fail(BP_ERR_VERIFY, "%s does not verify: %s", what, why.c_str());
  }
  return BP_OK;
}

int verify_child(const bp_state* s, const Box& b, const char* what, const uint8_t* bytes, size_t len) {
  return produced_here(s, bytes, len) ? BP_OK : verify_foreign(s, b, what);
}

// A job's finished proof words become its container -- this state's own, like every container it emits.
int box_of_job(const bp_state* s, const RecJob& job, const std::vector<uint64_t>& words, TreeBuf* out) {
  if (int r = emit_box(job.kind, CIRCUIT_ROOT + job.kind, job.pi, words, &out->p, &out->n)) return r;
  remember_proof(s, out->p, out->n);
  return BP_OK;
}
// ... and, for a rider, go back to the pool it was taken from
int finish_job(const bp_state* s, const RecJob& job, const std::vector<uint64_t>& words, RecPool* pool) {
  TreeBuf b;
  if (int r = box_of_job(s, job, words, &b)) return r;
  pool->complete(job, b.p, b.n);
  return BP_OK;
}

}  // namespace

extern "C" {

void bp_config_default(bp_config* c) {
  // constants.rs:6-18, positional order of prover_state.rs:85-93
  static const uint32_t lo[BP_NUM_TABLES] = {16, 9, 12, 14, 9, 12, 17}, hi[BP_NUM_TABLES] = {28, 28, 28, 25, 25, 28, 30};
  std::memset(c, 0, sizeof(*c));
  for (int t = 0; t < BP_NUM_TABLES; t++) { c->table_log_lo[t] = lo[t]; c->table_log_hi[t] = hi[t]; }
  c->stark_rate_bits = 1; c->stark_cap_height = 4; c->stark_num_queries = 84; c->stark_pow_bits = 16;
  c->arity_bits = 4; c->final_poly_bits = 5;
  // recursion-shaped proofs: proofs of the PLONK-shaped circuit (AIR 8), 135 wires, 85 preprocessed constant columns
  c->rec_log_n = 13; c->rec_n_cols = 135; c->rec_n_const = 85; c->rec_rate_bits = 3; c->rec_num_queries = 28;
  c->rec_pow_bits = 16;
  c->shrink_depth = 3;
  c->rec_air_id = 8;
  c->device = 0; c->n_workers = 4; c->arena_bytes = (uint64_t)6 << 30;
}

int bp_state_build(const bp_config* cfg, bp_state** out) try {
  if (!cfg || !out) return fail(BP_ERR_INVALID_INPUT, "bp_state_build: null argument");
  *out = nullptr;
  const StarkCfg rc = rec_cfg_of(*cfg);
  int r = check_cfg(rc);
  if (r) return r;
  if (cfg->shrink_depth < 1)
    return fail(BP_ERR_INVALID_INPUT, "shrink_depth must be at least 1: the root circuit walks Merkle paths of the recursion shape's depth, "
                "so its children are recursion-shaped proofs, not the tables' STARK proofs");
  uint32_t n_circ = 0;
  for (int t = 0; t < BP_NUM_TABLES; t++) {
    if (cfg->table_log_lo[t] >= cfg->table_log_hi[t] || cfg->table_log_hi[t] > 31)
      return fail(BP_ERR_INVALID_INPUT, "empty or invalid range for table %s", TABLES[t].name);
    StarkCfg tc = table_cfg_of(*cfg, cfg->table_log_lo[t], 8);
    if ((r = check_cfg(tc))) return r;
    n_circ += cfg->table_log_hi[t] - cfg->table_log_lo[t];
  }
  // Every recursion circuit walks one Merkle path per child: root (seven chains), aggregation (two children: their
  // paths' words follow the digests and flags), block (the aggregation child's), a table's shrink circuit (the level below)
  const uint32_t depth = rc.log_n + rc.rate_bits - rc.cap_height;
  // Every circuit whose children are recursion-shaped proofs (all but level 0 of a chain, whose child is a table's STARK
  // proof of up to 2432 columns) also HASHES the row each child opens (its leaf: the child's n_cols trace values) before
  // it walks up from it -- merkle_proofs::verify_merkle_proof_to_cap whole -- where the circuit has the rows for it (a
  // 2^6-row test circuit has them for one child, not for seven: both sides take the same decision from the shape alone)
  auto with_leaf = [&](air::plonk::Layout lay) {
    air::plonk::Layout l = lay;
    l.leaf_len = rc.n_cols;
    return (rc.air_id == air::PLONK && air::plonk::layout_ok(l, 1u << rc.log_n)) ? l : lay;
  };
  air::plonk::Layout special[3] = {with_leaf({ROOT_PATH_PI0 + 8 * BP_NUM_TABLES + BP_PV_WORDS, BP_NUM_TABLES, depth, ROOT_PATH_PI0}),
                                   with_leaf({AGG_PATH_PI0 + 2 * 8 + BP_PV_WORDS, 2, depth, AGG_PATH_PI0}),
                                   with_leaf({BLOCK_PATH_PI0 + 8 + BP_PV_WORDS, 1, depth, BLOCK_PATH_PI0})};
  const air::plonk::Layout shrink_lay = with_leaf(air::plonk::Layout{CHAIN_PATH_PI0 + 8, 1, depth, CHAIN_PATH_PI0});
  // ... and every circuit's rows must fit 2^rec_log_n: said here, from the shapes alone, before any device is looked for
  // (launch_plonk_constants would refuse the same layouts, after the arenas are allocated)
  if (rc.air_id == air::PLONK) {
    for (int t = 0; t < BP_NUM_TABLES; t++)
      for (uint32_t d = cfg->table_log_lo[t]; d < cfg->table_log_hi[t]; d++)
        if (!air::plonk::layout_ok(air::plonk::Layout{CHAIN_PATH_PI0 + 8, 1, d + cfg->stark_rate_bits - cfg->stark_cap_height, CHAIN_PATH_PI0}, 1u << rc.log_n))
          return fail(BP_ERR_INVALID_INPUT, "table %s at 2^%u rows: a Merkle path of %u levels (cap_height %u) does not fit the recursion circuit of 2^%u rows",
                      TABLES[t].name, d, d + cfg->stark_rate_bits - cfg->stark_cap_height, cfg->stark_cap_height, rc.log_n);
    const air::plonk::Layout all[4] = {special[0], special[1], special[2], shrink_lay};
    for (const air::plonk::Layout& l : all)
      if (!air::plonk::layout_ok(l, 1u << rc.log_n))
        return fail(BP_ERR_INVALID_INPUT, "the recursion shape's Merkle rows (%u paths of %u levels: log_n %u + rate_bits %u - cap_height %u) do not fit "
                    "a circuit of 2^%u rows", l.n_paths, l.depth, rc.log_n, rc.rate_bits, rc.cap_height, rc.log_n);
  }
  if (cfg->n_workers == 0 || cfg->n_workers > 64) return fail(BP_ERR_INVALID_INPUT, "n_workers out of range");
  int n_dev = bp_device_count();
  if (n_dev <= 0) return fail(BP_ERR_DEVICE, "no HIP device visible: the hot path has no CPU fallback");
  if (cfg->device < 0 || cfg->device >= n_dev) return fail(BP_ERR_DEVICE, "device %d not present", cfg->device);
  // prover threads must sleep, not spin, while they wait (capi.cpp); a refusal (context configured by
  // another library already) is not an error: the prover then works with spinning waits
  (void)bp_use_blocking_sync(cfg->device);
  std::unique_ptr<bp_state> s(new bp_state());
  s->cfg = *cfg;
  s->rec_cfg = rc;
  // persistent memory: per circuit K*n values + K*n coeffs + K*m LDE + digests
  const uint64_t N = (uint64_t)1 << rc.log_n, M = N << rc.rate_bits;
  const size_t per = ((size_t)rc.n_const * (2 * N + M) + 2 * M * 4 + 4096) * 8;
  const size_t circuits_bytes = per * (n_circ + 3 + BP_NUM_TABLES) + (64u << 20);
  {
    // size the whole state against the device BEFORE the first allocation: a late hipMalloc failure would name one
    // arena, not the configuration that does not fit
    (void)hipSetDevice(cfg->device);
    size_t free_b = 0, total_b = 0;
    BPG_HIP(hipMemGetInfo(&free_b, &total_b));
    const double need = (double)circuits_bytes + (double)cfg->n_workers * (double)cfg->arena_bytes;
    if (need > (double)free_b)
      return fail(BP_ERR_DEVICE,
                  "prover state does not fit device %d: %u preprocessed circuits %.1f GiB + %u prover arenas x %.1f GiB = "
                  "%.1f GiB, %.1f GiB free of %.1f GiB (lower n_workers or arena_bytes, or narrow the table ranges)",
                  cfg->device, n_circ + 3 + BP_NUM_TABLES, circuits_bytes / 1073741824.0, cfg->n_workers,
                  cfg->arena_bytes / 1073741824.0, need / 1073741824.0, free_b / 1073741824.0, total_b / 1073741824.0);
  }
  // from here on device memory is owned by *s: release it on every early return
  struct Unbuild {
    std::unique_ptr<bp_state>& s;
    ~Unbuild() {
      if (!s) return;
      for (auto& w : s->workers) w->destroy();
      for (void* p : s->slabs) (void)hipFree(p);
      s->builder.destroy();
    }
  } unbuild{s};
  if ((r = s->builder.init(cfg->device, circuits_bytes))) return r;
  s->table_circuits.resize(n_circ);
  uint32_t idx = 0;
  for (int t = 0; t < BP_NUM_TABLES; t++) {
    s->table_offset[t] = idx;
    for (uint32_t d = cfg->table_log_lo[t]; d < cfg->table_log_hi[t]; d++, idx++)
      // (digest, table, level) and the child's (leaf digest, cap entry): the child of level 0 is the table's STARK proof,
      // whose trace tree has d + rate - cap levels below its cap
      if ((r = build_circuit(s->builder, rc, circuit_seed(t, d),
                             air::plonk::Layout{CHAIN_PATH_PI0 + 8, 1, d + cfg->stark_rate_bits - cfg->stark_cap_height, CHAIN_PATH_PI0},
                             &s->table_circuits[idx]))) return r;
  }
  for (int t = 0; t < BP_NUM_TABLES; t++)
    if ((r = build_circuit(s->builder, rc, circuit_seed(t, SHRINK_SEED_DEGREE), shrink_lay,
                           &s->shrink_circuits[t]))) return r;
  for (uint32_t k = 0; k < 3; k++)
    if ((r = build_circuit(s->builder, rc, circuit_seed(CIRCUIT_ROOT + k, 0), special[k], &s->special[k]))) return r;
  BPG_HIP(hipStreamSynchronize(s->builder.stream));
  {
    // The arenas: one allocation cut into n_workers slices, so that neighbours can be leased as one piece of memory.
    // Where the device does not grant one allocation of that size the run is halved until it does: a few slabs, each
    // holding a whole run of slices (a slab of one slice is what every worker had before).
    s->slice_stride = ((size_t)cfg->arena_bytes + 255) & ~(size_t)255;
    std::vector<uint32_t> slab_of;
    for (uint32_t done = 0, run = cfg->n_workers; done < cfg->n_workers;) {
      run = std::min(run, cfg->n_workers - done);
      void* slab = nullptr;
      const hipError_t e = hipMalloc(&slab, (size_t)(run - 1) * s->slice_stride + cfg->arena_bytes);
      if (e != hipSuccess) {
        (void)hipGetLastError();
        if (run == 1) return fail(BP_ERR_DEVICE, "hipMalloc of a prover arena (%zu MiB) failed: %s", (size_t)cfg->arena_bytes >> 20, hipGetErrorString(e));
        run = (run + 1) / 2;
        continue;
      }
      s->slabs.push_back(slab);
      for (uint32_t k = 0; k < run; k++) {
        std::unique_ptr<Worker> w(new Worker());
        if ((r = w->init(cfg->device, cfg->arena_bytes, static_cast<char*>(slab) + (size_t)k * s->slice_stride))) { w->destroy(); return r; }
        s->workers.push_back(std::move(w));
        slab_of.push_back((uint32_t)s->slabs.size() - 1);
      }
      done += run;
    }
    s->table.reset(std::move(slab_of));
  }
  {
    // One prover = one HIP stream, and ROCm multiplexes a process's streams over GPU_MAX_HW_QUEUES hardware queues
    // (4 when unset), read once when the HIP runtime starts: provers beyond that number share a queue and run one
    // after the other -- the state works, at a fraction of its rate.  The library cannot raise the limit after the
    // runtime has started, so it says so.
    const char* env = std::getenv("GPU_MAX_HW_QUEUES");
    const long queues = env && *env ? std::strtol(env, nullptr, 10) : 4;
    // With fewer queues than streams the launches of a table proof are what the streams queue up behind: three
    // transactions' table proofs in lock-step (tune.hpp has the measurement); with a queue per stream one at a time.
    s->auto_txn_group = queues < (long)cfg->n_workers ? 3 : 1;
    if (queues < (long)cfg->n_workers) {
      char buf[512];
      std::snprintf(buf, sizeof(buf),
                    "GPU_MAX_HW_QUEUES is %s%ld but this state has %u prover streams: HIP maps a process's streams onto that many "
                    "hardware queues, so concurrent bp_generate_* calls beyond it serialise (measured: 16 streams on 4 queues run at "
                    "about half the rate).  Set GPU_MAX_HW_QUEUES >= n_workers (bench.py uses 32) in the environment BEFORE the process "
                    "makes its first HIP call.",
                    env && *env ? "" : "unset = ", queues, cfg->n_workers);
      s->warnings = buf;
    }
    if (bp_host_wait_mode(cfg->device) == 2) {
      if (!s->warnings.empty()) s->warnings += "\n";
      s->warnings += "The process had used this device before the library's first call, so the device's host-wait mode was left alone "
                     "(bp_use_blocking_sync); the library's prover threads wait with their own poll-and-sleep loop instead of the "
                     "runtime's spinning wait.  Nothing to do; call bp_use_blocking_sync(device) first thing for interrupt-driven waits.";
    }
  }
  *out = s.release();
  return BP_OK;
}
BPG_ABI_CATCH("bp_state_build")

const char* bp_state_warnings(const bp_state* s) { return s ? s->warnings.c_str() : ""; }
int bp_state_config(const bp_state* s, bp_config* out) {
  if (!s || !out) return fail(BP_ERR_INVALID_INPUT, "bp_state_config: null argument");
  *out = s->cfg;
  return BP_OK;
}

void bp_state_free(bp_state* s) {
  if (!s) return;
  (void)hipSetDevice(s->cfg.device);
  for (auto& w : s->workers) w->destroy();
  for (void* p : s->slabs) (void)hipFree(p);
  s->builder.destroy();
  delete s;
}

uint64_t bp_state_device_bytes(const bp_state* s) {
  if (!s) return 0;
  return s->builder.arena.capacity() + (uint64_t)s->workers.size() * s->cfg.arena_bytes;
}

// root_after of one txn (the synthetic "state transition"): hash_no_pad(root_before, seed, txn_number).
// Host-side, like the decoder that chains GenerationInputs in the reference (decoding.rs:106-154).
int bp_state_root_after(const uint64_t root_before[4], uint64_t seed, uint64_t txn_number, uint64_t out[4]) {
  if (!root_before || !out) return fail(BP_ERR_INVALID_INPUT, "bp_state_root_after: null argument");
  for (int i = 0; i < 4; i++) if (root_before[i] >= gl::P) return fail(BP_ERR_INVALID_INPUT, "non-canonical state root");
  root_after(root_before, seed, txn_number, out);
  return BP_OK;
}

int bp_proof_public_values(const uint8_t* proof, size_t len, uint64_t pv_out[BP_PV_WORDS], int* kind_out) try {
  if (!proof || len % 8 || len < (BOX_HDR + BP_PV_WORDS) * 8) return fail(BP_ERR_INVALID_INPUT, "proof: truncated");
  const uint64_t* w = reinterpret_cast<const uint64_t*>(proof);
  if (w[0] != PROOF_BOX_MAGIC || w[1] > 2 || w[2] < BP_PV_WORDS || w[2] > air::plonk::MAX_PI || len / 8 < BOX_HDR + w[2])
    return fail(BP_ERR_INVALID_INPUT, "proof: bad header");
  if (pv_out) std::memcpy(pv_out, w + BOX_HDR + w[2] - BP_PV_WORDS, BP_PV_WORDS * 8);
  if (kind_out) *kind_out = (int)w[1];
  return BP_OK;
}
BPG_ABI_CATCH("bp_proof_public_values")

// What upstream's `prove` returns before the recursion starts (AllProof: the seven table proofs, the lookup
// challenges, the public values) -- kept by bp_generate_txn_table_proofs, digested by bp_generate_txn_proof.
struct TableProofs {
  StarkCfg tcfg[BP_NUM_TABLES];
  std::vector<uint64_t> pv;
  Ctl ctl;
  std::vector<uint64_t> proof[BP_NUM_TABLES];
  uint64_t first_leaf[BP_NUM_TABLES][4];  // per table proof: the digest of the trace leaf its first query opens (stark_prove)
};
// generate_traces: the seven witnesses of a transaction in the worker's arena (d_trace[t]: n_cols x 2^log_n, column-major).
// What is to be made, and the refusals of data that cannot form one statement, are plan_traces' (txn_tables.cpp); here
// are the allocations, the staging and the launches.  Shared by the prover and the witness pre-flight.
// d_trace: allocated by the caller (alloc_traces).  stage: the worker whose pinned buffer the caller's items are staged
// through -- w itself, or for a group's transactions the worker each of them has leased.
static int build_traces(Worker& w, const Worker& stage, const uint64_t* I, const TxnWitness* wit, const StarkCfg tcfg[BP_NUM_TABLES],
                        uint64_t* const d_trace[BP_NUM_TABLES]) {
  int r;
  uint64_t* const pinned = stage.pinned;
  const size_t pinned_words = stage.pinned_words;
  bool given[BP_NUM_TABLES];
  size_t n_given[BP_NUM_TABLES];
  for (int t = 0; t < BP_NUM_TABLES; t++) {
    given[t] = given_table(wit, tcfg, t);
    n_given[t] = given[t] ? wit->n[t] : 0;
  }
  TracePlan plan;
  if ((r = plan_traces(tcfg, given, n_given, &plan))) return r;
  const bool lookup_kf = plan.lookup[L_SPONGE_KECCAK], lookup_bm = plan.lookup[L_PACKING_MEMORY], lookup_sl = plan.lookup[L_SPONGE_LOGIC];
  // a looking table before the table it looks up (sponge before Keccak-f, byte packing before memory)
  static const int GEN_ORDER[BP_NUM_TABLES] = {T_KECCAK_SPONGE, T_ARITHMETIC, T_BYTE_PACKING, T_CPU, T_KECCAK, T_LOGIC, T_MEMORY};
  const uint64_t* d_sponge = d_trace[T_KECCAK_SPONGE];
  const uint32_t sponge_log_n = tcfg[T_KECCAK_SPONGE].log_n;
  const uint64_t sponge_N = (uint64_t)1 << sponge_log_n;
  for (int gi = 0; gi < BP_NUM_TABLES; gi++) {
    const int t = GEN_ORDER[gi];
    const uint64_t N = (uint64_t)1 << tcfg[t].log_n, seed = I[10] ^ splitmix64(t + 1);
    const size_t wds = TABLES[t].item_words, cap = witness_capacity(t, N);
    const size_t mark = w.arena.mark();
    uint64_t* d_in = nullptr;
    if (t == T_LOGIC && lookup_sl) {
      // [five operations per covered sponge row][the caller's operations, or seeded ones]
      const size_t n_ops = n_given[t], covered = (size_t)air::ctl::SPONGE_LOGIC_OPS * plan.logic_covered;
      d_in = w.arena.alloc_words((size_t)N * wds + n_ops * wds);
      if (!d_in) return fail(BP_ERR_DEVICE, "device arena exhausted for the logic table's operations");
      uint64_t* d_given = nullptr;
      if (n_ops) {
        if (n_ops * wds > pinned_words) return fail(BP_ERR_UNSUPPORTED, "too many logic operations for the input staging buffer");
        std::memcpy(pinned, wit->in[t], n_ops * wds * 8);
        d_given = d_in + (size_t)N * wds;
        BPG_HIP(hipMemcpyAsync(d_given, pinned, n_ops * wds * 8, hipMemcpyHostToDevice, w.stream));
      }
      if ((r = launch_logic_inputs_from_sponge(d_sponge, sponge_log_n, plan.logic_covered, given[t] ? d_given : nullptr, (uint32_t)n_ops,
                                               d_in, (uint32_t)N, seed, w.stream))) return r;
      if (given[t] && !d_given) {  // an empty list was given: padding operations, not seeded ones
        BPG_HIP(hipMemsetAsync(d_in + covered * wds, 0, ((size_t)N - covered) * wds * 8, w.stream));
      }
    } else if (given[t]) {
      // the caller's items, then padding up to the table's height, staged through the pinned buffer
      const size_t words = cap * wds;
      d_in = w.arena.alloc_words(words);
      if (!d_in) return fail(BP_ERR_DEVICE, "device arena exhausted for the witness data of table %s", TABLES[t].name);
      if (words > pinned_words) return fail(BP_ERR_UNSUPPORTED, "table %s too tall for the input staging buffer", TABLES[t].name);
      fill_table_inputs(t, N, wit->in[t], wit->n[t], pinned);
      BPG_HIP(hipMemcpyAsync(d_in, pinned, words * 8, hipMemcpyHostToDevice, w.stream));
    } else if (t == T_KECCAK && lookup_kf) {
      d_in = w.arena.alloc_words(cap * wds);
      if (!d_in) return fail(BP_ERR_DEVICE, "device arena exhausted for the Keccak-f table's inputs");
      if ((r = launch_keccak_inputs_from_sponge(d_sponge, sponge_log_n, d_in, (uint32_t)cap, seed, w.stream))) return r;
    } else if (t == T_MEMORY && lookup_bm) {
      d_in = w.arena.alloc_words((size_t)N * wds);
      if (!d_in) return fail(BP_ERR_DEVICE, "device arena exhausted for the memory table's log");
      if ((r = launch_memory_inputs_from_byte_packing(d_trace[T_BYTE_PACKING], tcfg[T_BYTE_PACKING].log_n, d_in, (uint32_t)N, w.stream))) return r;
    }
    r = tcfg[t].air_id == air::SYNTHETIC
            ? launch_synth_trace(d_trace[t], nullptr, tcfg[t].log_n, tcfg[t].n_cols, 0, 1, seed, w.stream)
            : launch_air_trace(tcfg[t].air_id, d_trace[t], d_in, tcfg[t].log_n, d_in ? 0 : seed, w.stream, plan.sponge_row_limit);
    if (r) return r;
    // the filter column of a looked table (air::ctl) is part of its TRACE: written here, committed with the trace, i.e.
    // before the lookup challenges are drawn.  The looking table's trace is there already (GEN_ORDER).
    if (t == T_KECCAK && lookup_kf) {  // the permutations the sponge table asks for: its flag columns, row p <-> permutation p
      r = launch_lookup_filter(air::KECCAK_F, d_trace[t], tcfg[t].log_n, d_sponge + (size_t)air::keccak_sponge::COL_FULL * sponge_N,
                               d_sponge + (size_t)air::keccak_sponge::COL_FINAL * sponge_N, (uint32_t)sponge_N, w.stream);
    } else if (t == T_MEMORY && lookup_bm) {  // the operations the byte-packing table looks up: its trace (address, timestamp per row)
      r = launch_lookup_filter(air::MEMORY, d_trace[t], tcfg[t].log_n, d_trace[T_BYTE_PACKING], nullptr, (uint32_t)1 << tcfg[T_BYTE_PACKING].log_n, w.stream);
    } else if (t == T_LOGIC && lookup_sl) {  // the XORs the sponge table asks for: rows 5 p + m of the rows p that absorb a block
      r = launch_lookup_filter(air::LOGIC, d_trace[t], tcfg[t].log_n, d_sponge + (size_t)air::keccak_sponge::COL_FULL * sponge_N,
                               d_sponge + (size_t)air::keccak_sponge::COL_FINAL * sponge_N, plan.logic_covered, w.stream);
    }
    if (r) return r;
    if (d_in) {  // the staging buffer and the input words are reused by the next table
      if ((r = w.wait())) return r;
      w.arena.release(mark);
    }
  }
  return BP_OK;
}

// The seven table proofs as bp_generate_txn_table_proofs hands them out:
// "BPGTABLS" | n_tables | public values | lookup challenges | per table: air_id, log_n, n_cols, n_words, proof words
static int emit_tables(const TableProofs& tp, uint8_t** out, size_t* out_len) {
  const StarkCfg* tcfg = tp.tcfg;
  const std::vector<uint64_t>& pv = tp.pv;
  std::vector<uint64_t> o = {TABLES_MAGIC, BP_NUM_TABLES};
  o.insert(o.end(), pv.begin(), pv.end());
  o.insert(o.end(), tp.ctl.v, tp.ctl.v + 4);
  for (int t = 0; t < BP_NUM_TABLES; t++) {
    const uint64_t hdr[4] = {tcfg[t].air_id, tcfg[t].log_n, tcfg[t].n_cols, tp.proof[t].size()};
    o.insert(o.end(), hdr, hdr + 4);
    o.insert(o.end(), tp.proof[t].begin(), tp.proof[t].end());
  }
  uint64_t* buf = static_cast<uint64_t*>(std::malloc(o.size() * 8));
  if (!buf) return fail(BP_ERR_DEVICE, "host allocation failed");
  std::memcpy(buf, o.data(), o.size() * 8);
  *out = reinterpret_cast<uint8_t*>(buf);
  *out_len = o.size() * 8;
  return BP_OK;
}

// What follows the table proofs of the g transactions of a group (g = 1: a lone transaction): the recursion chains over
// them and each transaction's root proof (or, with a pool, the root posted as the job of nodes[i]).  The traces are
// dead: the arena goes back to `arena_mark`.
static int group_recursion(const bp_state* s, Worker& w, size_t arena_mark, TableProofs* const* tps, uint32_t g, uint8_t** outs,
                           size_t* out_lens, RecPool* pool, const uint32_t* nodes) {
  const bp_config& cfg = s->cfg;
  constexpr uint32_t T = BP_NUM_TABLES;
  const uint32_t n_chains = T * g;
  int r;
  // per child of a recursion circuit: its digest, and the Merkle path of its first trace opening (leaf digest, cap entry:
  // words of the parent's public-input list; position and siblings: witness of the parent's Merkle rows).  Slot T i + t:
  // chain t of transaction i.
  struct Child {
    uint64_t digest[4], leaf_cap[8];
  };
  std::vector<Child> child(n_chains);
  std::vector<std::vector<PathWitness>> slot_path(n_chains);
  for (uint32_t i = 0; i < g; i++) {
    TableProofs& tp = *tps[i];
    for (uint32_t t = 0; t < T; t++) {
      Child& c = child[T * i + t];
      proof_digest(tp.tcfg[t], tp.proof[t].data(), c.digest);
      slot_path[T * i + t].resize(1);
      first_query_trace_path(tp.tcfg[t], tp.proof[t].data(), c.leaf_cap, c.leaf_cap + 4, &slot_path[T * i + t][0], tp.first_leaf[t]);
      std::vector<uint64_t>().swap(tp.proof[t]);
    }
  }
  if ((r = w.wait())) return r;
  w.arena.release(arena_mark);  // traces are dead; the chains below only need digests
  // per-table recursion-shaped chains (wrap + shrinks).  The chains do not depend on each other and their proofs have
  // one shape: level k of all seven chains of all g transactions is ONE batch proved in lock-step (rec_prove_batch) --
  // 7 g transcripts stepped together, every kernel launch and host wait shared, every grid g times as large --, then
  // level k + 1.  (Until round 4 each chain was its own sequence of 6..16-column launches: 88 of a transaction's 118 LDE
  // launches and most of its 1,620 kernel launches; until Tune::rec_group each transaction of a group ran its levels
  // alone, the group's other provers idle.)  Level 0 is proved by the circuit of the table's height (its child is the
  // table's STARK proof), the levels above by the table's shrink circuit.
  // With a pool (a shard's scheduler, gi.cpp) each of these batches also carries ready jobs of the pool -- other
  // transactions' root proofs, the tree's aggregation proofs -- in the slots the chains leave free: one more circuit,
  // list and transcript in launches that are made anyway.  A rider's container is handed back the moment its batch is
  // done; a state whose batches have no room beyond the chains carries none.
  {
    const uint32_t cap = lockstep_cap(s->rec_cfg, w.pinned_words, g);
    std::vector<const Circuit*> circ(n_chains);
    std::vector<std::vector<uint64_t>> pis(n_chains), chain_proof;
    for (uint32_t depth = 0; depth < cfg.shrink_depth; depth++) {
      if (w.aborted()) return fail(BP_ERR_ABORTED, "aborted in the recursion chains (level %u)", depth);
      for (uint32_t i = 0; i < g; i++)
        for (uint32_t t = 0; t < T; t++) {
          const Child& c = child[T * i + t];
          circ[T * i + t] = depth == 0 ? &s->table_circuits[s->table_offset[t] + (tps[i]->tcfg[t].log_n - cfg.table_log_lo[t])] : &s->shrink_circuits[t];
          pis[T * i + t] = {c.digest[0], c.digest[1], c.digest[2], c.digest[3], (uint64_t)t, depth};
          pis[T * i + t].insert(pis[T * i + t].end(), c.leaf_cap, c.leaf_cap + 8);
        }
      std::vector<std::unique_ptr<RecJob>> riders;
      if (pool && cap > n_chains) pool->take(cap - n_chains, &riders);
      const uint32_t n = n_chains + (uint32_t)riders.size();
      circ.resize(n); pis.resize(n); slot_path.resize(n);
      for (size_t k = 0; k < riders.size(); k++) {
        circ[n_chains + k] = static_cast<const Circuit*>(riders[k]->circuit);
        pis[n_chains + k] = riders[k]->pi;
        slot_path[n_chains + k] = std::move(riders[k]->paths);
      }
      chain_proof.assign(n, {});
      std::vector<uint64_t> first_leaf(4 * (size_t)n);
      if ((r = rec_prove_batch(w, s->rec_cfg, n, circ.data(), pis.data(), chain_proof.data(), slot_path.data(), first_leaf.data(), g))) return r;
      for (size_t k = 0; k < riders.size(); k++)
        if ((r = finish_job(s, *riders[k], chain_proof[n_chains + k], pool))) return r;
      for (uint32_t k = 0; k < n_chains; k++) {
        proof_digest(s->rec_cfg, chain_proof[k].data(), child[k].digest);
        first_query_trace_path(s->rec_cfg, chain_proof[k].data(), child[k].leaf_cap, child[k].leaf_cap + 4, &slot_path[k][0], &first_leaf[4 * k]);
      }
    }
  }
  // root proofs: a transaction's seven chain digests, their seven (leaf digest, cap entry) pairs, its public values
  for (uint32_t i = 0; i < g; i++) {
    std::vector<uint64_t> pi;
    std::vector<PathWitness> root_paths(T);
    for (uint32_t t = 0; t < T; t++) pi.insert(pi.end(), child[T * i + t].digest, child[T * i + t].digest + 4);
    for (uint32_t t = 0; t < T; t++) {
      pi.insert(pi.end(), child[T * i + t].leaf_cap, child[T * i + t].leaf_cap + 8);
      root_paths[t] = std::move(slot_path[T * i + t][0]);
    }
    pi.insert(pi.end(), tps[i]->pv.begin(), tps[i]->pv.end());
    if (pool) {  // the root rides in another transaction's batch, or in a batch of the jobs that are left at the end
      std::unique_ptr<RecJob> job(new RecJob());
      job->node = nodes ? nodes[i] : 0;
      job->kind = 0;
      job->circuit = &s->special[0];
      job->pi = std::move(pi);
      job->paths = std::move(root_paths);
      pool->post(std::move(job));
      continue;
    }
    std::vector<uint64_t> proof;
    if ((r = rec_prove(w, s->rec_cfg, s->special[0], pi, proof, &root_paths))) return r;
    if ((r = emit_box(0, CIRCUIT_ROOT, pi, proof, &outs[i], &out_lens[i]))) return r;
    remember_proof(s, outs[i], out_lens[i]);
  }
  return BP_OK;
}

// ---- several transactions at a time (Tune::txn_group) ----------------------------------------------------------------
// The seven tables of ONE transaction share a transcript and cannot be stepped together; table t of transaction A and
// table t of transaction B have separate transcripts and, wherever their heights agree, one shape.  A prover that holds
// a group of transactions therefore proves table t of all of them as lock-step batches (stark_prove_batch, the
// machinery of the recursion chains), t = 0..6 in order, each transaction on its own transcript: the ~57 launches and
// ~15 host waits of a table proof are paid once per batch instead of once per transaction.
namespace {

struct GroupTxn {  // one transaction of a group
  const uint64_t* I = nullptr;
  const TxnWitness* wit = nullptr;
  TableProofs tp;
};

bool same_shape(const StarkCfg& a, const StarkCfg& b) {
  return a.log_n == b.log_n && a.n_cols == b.n_cols && a.n_const == b.n_const && a.deg_pow == b.deg_pow && a.rate_bits == b.rate_bits &&
         a.cap_height == b.cap_height && a.num_queries == b.num_queries && a.pow_bits == b.pow_bits && a.arity_bits == b.arity_bits &&
         a.final_poly_bits == b.final_poly_bits && a.air_id == b.air_id;
}
// Table proofs of shape c one lock-step batch holds: every limit stark_prove_batch and commit_batch would refuse at,
// taken up front so that a sub-batch is SPLIT and never failed -- MAX_BATCH (a group holds eight transactions at
// most), the query launches' index limit (MAX_BATCH_QUERIES: 84 queries -> 8 proofs), and the mailbox (mailbox_cap).
uint32_t table_batch_cap(const StarkCfg& c, size_t pinned_words) {
  size_t cap = std::min<size_t>(MAX_BATCH, MAX_BATCH_QUERIES / std::max<uint32_t>(1, c.num_queries));
  cap = std::min(cap, mailbox_cap(c, pinned_words));
  return (uint32_t)std::max<size_t>(1, cap);
}

struct SubBatch {  // the transactions of a group whose table t has one shape, at most table_batch_cap of them
  uint32_t n = 0;
  uint32_t txn[MAX_BATCH];
  uint64_t* d_traces = nullptr;  // [n][n_cols][N]
};
struct TraceLayout {
  std::vector<SubBatch> subs[BP_NUM_TABLES];                      // per table, in the order of their first transaction
  std::vector<std::array<uint64_t*, BP_NUM_TABLES>> d_trace;      // per transaction: its place in its sub-batches
};
// The traces of g transactions in w's arena (tcfg[i]: the seven shapes of transaction i): table by table, the equally
// shaped traces of a sub-batch one behind the other, as commit_batch wants them.  A lone transaction's seven traces lie
// in table order.
int alloc_traces(Worker& w, const StarkCfg* const* tcfg, uint32_t g, TraceLayout* out) {
  out->d_trace.resize(g);
  for (int t = 0; t < BP_NUM_TABLES; t++) {
    std::vector<SubBatch>& subs = out->subs[t];
    for (uint32_t i = 0; i < g; i++) {
      const StarkCfg& c = tcfg[i][t];
      const uint32_t cap = table_batch_cap(c, w.pinned_words);
      SubBatch* sb = nullptr;
      for (auto& cand : subs)
        if (cand.n < cap && same_shape(tcfg[cand.txn[0]][t], c)) { sb = &cand; break; }
      if (!sb) { subs.emplace_back(); sb = &subs.back(); }
      sb->txn[sb->n++] = i;
    }
    for (auto& sb : subs) {
      const StarkCfg& c = tcfg[sb.txn[0]][t];
      const size_t words = (size_t)c.n_cols << c.log_n;
      sb.d_traces = w.arena.alloc_words(words * sb.n);
      if (!sb.d_traces) return fail(BP_ERR_DEVICE, "device arena exhausted (%zu MiB) for table %s", w.arena.capacity() >> 20, TABLES[t].name);
      for (uint32_t k = 0; k < sb.n; k++) out->d_trace[sb.txn[k]][t] = sb.d_traces + k * words;
    }
  }
  return BP_OK;
}

// The trace commitments of a group (trace[i][t]: table t of transaction i): one commit_batch per sub-batch.
// The seven commitments of a transaction do not depend on each other.  Under load they queue on the prover's stream like
// everything else (the chip is full); a prover that is ALONE on the device with ONE transaction -- a lone call, the last
// one of a shard -- borrows the streams of up to three idle workers and the commitments overlap: the wide Keccak table's
// long sponge chains no longer have the chip to themselves (largest first, each to the lane with the least work so far).
// A group never takes lanes, whatever Tune::side_lanes says (it counts as the provers it holds).
int commit_traces(const bp_state* s, Worker& w, const StarkCfg* const* tcfg, const TraceLayout& lay,
                  std::array<Committed, BP_NUM_TABLES>* trace) {
  int r;
  std::vector<std::unique_ptr<SideLane>> sides;
  if (lay.d_trace.size() == 1 && provers_active() <= tune().side_lanes.load(std::memory_order_relaxed))
    for (int k = 0; k < 3; k++) {
      std::unique_ptr<SideLane> l = SideLane::try_acquire(s);
      if (!l) break;
      sides.push_back(std::move(l));
    }
  if (sides.empty()) {
    for (int t = 0; t < BP_NUM_TABLES; t++)
      for (const SubBatch& sb : lay.subs[t]) {
        const StarkCfg& c = tcfg[sb.txn[0]][t];
        Committed cm[MAX_BATCH];
        if ((r = commit_batch(w, sb.d_traces, c.n_cols, sb.n, c.log_n, c.rate_bits, c.cap_height, false, cm))) return r;
        for (uint32_t k = 0; k < sb.n; k++) trace[sb.txn[k]][t] = std::move(cm[k]);
      }
    return BP_OK;
  }
  const StarkCfg* c = tcfg[0];
  BPG_HIP(hipEventRecord(w.sync_event, w.stream));  // the witnesses are made on this prover's stream
  std::vector<Worker*> lane = {&w};
  for (auto& l : sides) {
    BPG_HIP(hipStreamWaitEvent(l->w->stream, w.sync_event, 0));
    lane.push_back(l->w);
  }
  std::vector<uint64_t> load(lane.size(), 0);
  std::vector<size_t> slots(lane.size(), 0);
  int order[BP_NUM_TABLES];
  for (int t = 0; t < BP_NUM_TABLES; t++) order[t] = t;
  auto cells = [&](int t) { return (uint64_t)c[t].n_cols << c[t].log_n; };
  std::sort(order, order + BP_NUM_TABLES, [&](int a, int b) { return cells(a) != cells(b) ? cells(a) > cells(b) : a < b; });
  PendingCommit pc[BP_NUM_TABLES];
  for (int oi = 0; oi < BP_NUM_TABLES; oi++) {
    const int t = order[oi];
    const size_t k = std::min_element(load.begin(), load.end()) - load.begin();
    if ((r = commit_launch(w, *lane[k], slots[k], lay.d_trace[0][t], c[t].n_cols, 1, c[t].log_n, c[t].rate_bits, c[t].cap_height, false, &pc[t])))
      return r;
    load[k] += cells(t);
    slots[k] += (size_t)4 << c[t].cap_height;
  }
  for (int t = 0; t < BP_NUM_TABLES; t++)
    if ((r = commit_finish(pc[t], &trace[0][t]))) return r;
  return BP_OK;  // the lanes are drained (commit_finish waited for each): back to their owners
}

// generate_traces + the seven table proofs of each of g >= 1 transactions (plonky2_evm `prove`), on the lease's leading
// worker (its arena spans the group's slices); stage[i]: the worker transaction i stages its witness data through
int prove_tables(const bp_state* s, Worker& w, const std::vector<Worker*>& stage, GroupTxn* const* tx, uint32_t g) {
  int r;
  std::vector<const StarkCfg*> tcfg(g);
  for (uint32_t i = 0; i < g; i++) tcfg[i] = tx[i]->tp.tcfg;
  TraceLayout lay;
  if ((r = alloc_traces(w, tcfg.data(), g, &lay))) return r;
  // generate_traces per transaction (its seed, plan and lookups)
  for (uint32_t i = 0; i < g; i++)
    if ((r = build_traces(w, *stage[i], tx[i]->I, tx[i]->wit, tcfg[i], lay.d_trace[i].data()))) return r;
  std::vector<std::array<Committed, BP_NUM_TABLES>> trace(g);
  if ((r = commit_traces(s, w, tcfg.data(), lay, trace.data()))) return r;
  // every transaction's own transcript: its seven caps, its public values, its lookup challenges
  std::vector<Challenger> ch(g);
  for (uint32_t i = 0; i < g; i++) {
    TableProofs& tp = tx[i]->tp;
    for (int t = 0; t < BP_NUM_TABLES; t++) ch[i].observe(trace[i][t].cap.data(), trace[i][t].cap.size());
    ch[i].observe(tp.pv.data(), tp.pv.size());
    for (int k = 0; k < 4; k++) tp.ctl.v[k] = ch[i].challenge();
  }
  // the table proofs: t = 0..6 in order (one transcript per transaction runs through its seven), table t of the
  // transactions of a sub-batch in lock-step
  for (int t = 0; t < BP_NUM_TABLES; t++)
    for (const SubBatch& sb : lay.subs[t]) {
      if (w.aborted()) return fail(BP_ERR_ABORTED, "aborted before table %s", TABLES[t].name);
      const StarkCfg& c = tcfg[sb.txn[0]][t];
      const size_t mark = w.arena.mark();
      Challenger before[MAX_BATCH], cur[MAX_BATCH];  // before: the transcript as the verifier of this table proof starts from it
      Committed tr[MAX_BATCH];
      const Committed* no_consts[MAX_BATCH] = {};
      const uint64_t* d_tv[MAX_BATCH];
      Ctl ctl[MAX_BATCH];
      std::vector<uint64_t> proofs[MAX_BATCH];
      uint64_t first_leaf[MAX_BATCH][4];
      for (uint32_t k = 0; k < sb.n; k++) {
        const uint32_t i = sb.txn[k];
        before[k] = cur[k] = ch[i];
        tr[k] = trace[i][t];
        d_tv[k] = lay.d_trace[i][t];
        ctl[k] = tx[i]->tp.ctl;
      }
      if ((r = stark_prove_batch(w, c, sb.n, no_consts, tr, d_tv, ctl, cur, proofs, &first_leaf[0][0]))) return r;
      for (uint32_t k = 0; k < sb.n; k++) {
        const uint32_t i = sb.txn[k];
        TableProofs& tp = tx[i]->tp;
        ch[i] = cur[k];
        tp.proof[t] = std::move(proofs[k]);
        std::memcpy(tp.first_leaf[t], first_leaf[k], 32);
        // The prover does not check a witness, and nothing downstream of this call verifies the table proofs (upstream's
        // root circuit would): data that came from the caller is therefore checked here, by the CPU verifier on the
        // proof just made -- a log that is not a memory, a block that is not padded, ... ends the call.
        if (given_table(tx[i]->wit, tp.tcfg, t) && stark_verify(c, nullptr, tp.ctl, before[k], tp.proof[t].data(), tp.proof[t].size()) != BP_OK) {
          const std::string why = bp_last_error();
          return fail(BP_ERR_VERIFY, "the witness data given for table %s does not satisfy its AIR: %s", TABLES[t].name, why.c_str());
        }
      }
      w.arena.release(mark);
    }
  // the tables of a transaction must be ONE statement: what the sponge table hashes is what the Keccak-f table permutes
  for (uint32_t i = 0; i < g; i++)
    if ((r = check_lookups(tx[i]->tp.tcfg, tx[i]->tp.proof))) return r;
  return BP_OK;
}

}  // namespace

// Up to n transactions on one lease -- a lone transaction is a group of one: as many as the lease grants (>= 1;
// `granted` hears the number the moment the lease is held, so that a scheduler can hand the others on), their table
// proofs in lock-step, then the recursion chains of all of them level by level in lock-step and each transaction's root
// (Tune::rec_group 1: each transaction's recursion and root, one transaction after the other), on the lease's stream.  outs / out_lens per transaction (tables_only: the table-proof blobs); with a pool the roots are
// posted as the jobs of nodes[i] instead.  The first failing transaction's status and message are the call's.
static int txn_proofs_impl(const bp_state* s, uint32_t n, const uint8_t* const* irs, size_t ir_len, const TxnWitness* const* wits,
                           const volatile int32_t* abort_flag, const volatile uint8_t* abort_flag_u8, bool tables_only, RecPool* pool,
                           const uint32_t* nodes, const std::function<void(uint32_t)>* granted, uint8_t** outs, size_t* out_lens,
                           uint32_t* n_done) {
  if (!s || !irs || !n || ((!outs || !out_lens) && !pool)) return fail(BP_ERR_INVALID_INPUT, "bp_generate_txn_proof: null argument");
  n = std::min<uint32_t>(n, MAX_BATCH);
  for (uint32_t i = 0; i < n; i++)
    if (!irs[i]) return fail(BP_ERR_INVALID_INPUT, "bp_generate_txn_proof: null argument");
  if (ir_len != BP_IR_WORDS * 8) return fail(BP_ERR_INVALID_INPUT, "IR must be %d bytes", BP_IR_WORDS * 8);
  (void)hipSetDevice(s->cfg.device);
  std::vector<std::unique_ptr<GroupTxn>> tx;
  ProverLease lease(s, n);
  const uint32_t g = lease.size();
  if (granted) (*granted)(g);
  if (n_done) *n_done = g;
  int r;
  std::vector<GroupTxn*> p;
  for (uint32_t i = 0; i < g; i++) {
    tx.emplace_back(new GroupTxn());
    p.push_back(tx[i].get());
    tx[i]->I = reinterpret_cast<const uint64_t*>(irs[i]);
    tx[i]->wit = wits ? wits[i] : nullptr;
    if ((r = parse_ir(s->cfg, tx[i]->I, tx[i]->wit, tx[i]->tp.tcfg, &tx[i]->tp.pv))) return r;
  }
  Worker& w = *lease.w;
  w.abort_flag = abort_flag;
  w.abort_flag_u8 = abort_flag_u8;
  if (w.aborted()) return fail(BP_ERR_ABORTED, "aborted before start");
  if ((r = prove_tables(s, w, lease.ws, p.data(), g))) return r;
  if (tables_only) {
    for (uint32_t i = 0; i < g; i++)
      if ((r = emit_tables(tx[i]->tp, &outs[i], &out_lens[i]))) return r;
    return BP_OK;
  }
  std::vector<TableProofs*> tps;
  for (uint32_t i = 0; i < g; i++) tps.push_back(&tx[i]->tp);
  if (tune().rec_group.load(std::memory_order_relaxed) != 1) return group_recursion(s, w, lease.mark, tps.data(), g, outs, out_lens, pool, nodes);
  for (uint32_t i = 0; i < g; i++)  // one transaction's recursion after the other
    if ((r = group_recursion(s, w, lease.mark, &tps[i], 1, outs ? outs + i : nullptr, out_lens ? out_lens + i : nullptr, pool, nodes ? nodes + i : nullptr))) return r;
  return BP_OK;
}
// the calls that take one IR: a group of one
static int txn_proof_of_one(const bp_state* s, const uint8_t* ir, size_t ir_len, const TxnWitness* wit, const volatile int32_t* abort_flag,
                            const volatile uint8_t* abort_flag_u8, bool tables_only, uint8_t** out, size_t* out_len) {
  return txn_proofs_impl(s, 1, &ir, ir_len, &wit, abort_flag, abort_flag_u8, tables_only, nullptr, nullptr, nullptr, out, out_len, nullptr);
}
int bp_generate_txn_proof(const bp_state* s, const uint8_t* ir, size_t ir_len, const volatile int32_t* abort_flag,
                          uint8_t** out, size_t* out_len) try {
  return txn_proof_of_one(s, ir, ir_len, nullptr, abort_flag, nullptr, false, out, out_len);
}
BPG_ABI_CATCH("bp_generate_txn_proof")
// rec_prove_batch's sub-batches by the proofs they held (include/bpg.h)
int bp_debug_rec_batch_histogram(uint64_t* out, uint32_t n, int reset) try {
  if (!out && n) return fail(BP_ERR_INVALID_INPUT, "bp_debug_rec_batch_histogram: null argument");
  std::atomic<uint64_t>* sizes = rec_batch_sizes();
  for (uint32_t b = 0; b <= MAX_LOCKSTEP; b++) {
    const uint64_t v = reset ? sizes[b].exchange(0) : sizes[b].load();
    if (b < n) out[b] = v;
  }
  for (uint32_t b = MAX_LOCKSTEP + 1; b < n; b++) out[b] = 0;
  return BP_OK;
}
BPG_ABI_CATCH("bp_debug_rec_batch_histogram")
// The same call with the reference's own flag type: Option<Arc<AtomicBool>> (proof_gen.rs:42) is one byte,
// `flag.as_ptr()` binds directly.
int bp_generate_txn_proof_u8(const bp_state* s, const uint8_t* ir, size_t ir_len, const volatile uint8_t* abort_flag,
                             uint8_t** out, size_t* out_len) try {
  return txn_proof_of_one(s, ir, ir_len, nullptr, nullptr, abort_flag, false, out, out_len);
}
BPG_ABI_CATCH("bp_generate_txn_proof_u8")
// generate_txn_proof where the transaction's Keccak table attests GIVEN hashing work: keccak_inputs = the states that
// go into its Keccak-f permutations (n_perms x 25 lanes, e.g. from bp_keccak256_permutation_inputs over the signed
// transaction and the contract code of its GenerationInputs).  abort_flag as in bp_generate_txn_proof_u8.
int bp_generate_txn_proof_keccak(const bp_state* s, const uint8_t* ir, size_t ir_len, const uint64_t* keccak_inputs,
                                 size_t n_perms, const volatile uint8_t* abort_flag, uint8_t** out, size_t* out_len) try {
  if (!keccak_inputs && n_perms) return fail(BP_ERR_INVALID_INPUT, "bp_generate_txn_proof_keccak: null inputs");
  TxnWitness wit;
  wit.give(T_KECCAK, keccak_inputs, n_perms);
  return txn_proof_of_one(s, ir, ir_len, &wit, nullptr, abort_flag, false, out, out_len);
}
BPG_ABI_CATCH("bp_generate_txn_proof_keccak")
// The general form: witness data for any of the tables that have an AIR (bp_txn_witness, include/bpg.h).
int bp_generate_txn_proof_witness(const bp_state* s, const uint8_t* ir, size_t ir_len, const bp_txn_witness* data,
                                  const volatile uint8_t* abort_flag, uint8_t** out, size_t* out_len) try {
  TxnWitness wit;
  if (int r = witness_of(data, &wit)) return r;
  return txn_proof_of_one(s, ir, ir_len, &wit, nullptr, abort_flag, false, out, out_len);
}
BPG_ABI_CATCH("bp_generate_txn_proof_witness")

// ---- the transaction witness pre-flight (bp_check_txn_witness) ----------------------------------------------------
static int check_txn_impl(const bp_state* s, const uint8_t* ir, size_t ir_len, const TxnWitness* wit, bp_witness_report* out) {
  if (!s || !ir || !out) return fail(BP_ERR_INVALID_INPUT, "bp_check_txn_witness: null argument");
  if (ir_len != BP_IR_WORDS * 8) return fail(BP_ERR_INVALID_INPUT, "IR must be %d bytes", BP_IR_WORDS * 8);
  std::memset(out, 0, sizeof(*out));
  const uint64_t* I = reinterpret_cast<const uint64_t*>(ir);
  StarkCfg tcfg[BP_NUM_TABLES];
  std::vector<uint64_t> pv;
  int r = parse_ir(s->cfg, I, wit, tcfg, &pv);
  if (r) return r;
  (void)hipSetDevice(s->cfg.device);
  ProverLease lease(s);
  Worker& w = *lease.w;
  w.abort_flag = nullptr;
  w.abort_flag_u8 = nullptr;
  struct Release { Worker& w; size_t mark; ~Release() { (void)w.wait(); w.arena.release(mark); } } rel{w, lease.mark};
  const StarkCfg* const one = tcfg;
  TraceLayout lay;
  if ((r = alloc_traces(w, &one, 1, &lay))) return r;
  uint64_t* const* d_trace = lay.d_trace[0].data();
  if ((r = build_traces(w, w, I, wit, tcfg, d_trace))) return r;
  if ((r = w.wait())) return r;
  // The tables proven by an AIR as contiguous caller tables (a synthetic table has no trace here: it is left alone), the
  // active lookups as links, on the worker's stream.  A seeded or derived table satisfies its AIR by construction; the
  // prover checks the given ones, so only those fail the call.
  CallerTable tables[BP_NUM_TABLES] = {};
  for (int t = 0; t < BP_NUM_TABLES; t++)
    if (tcfg[t].air_id != air::SYNTHETIC) tables[t] = caller_table(tcfg[t], d_trace[t], (uint64_t)1 << tcfg[t].log_n, nullptr, nullptr);
  bp_set_link links[air::ctl::N_PAIRS];
  uint32_t pair[air::ctl::N_PAIRS];
  const uint32_t n_links = links_of(tcfg, links, pair);
  bp_set_report found{};
  if ((r = check_tables_and_links("bp_check_txn_witness", tables, BP_NUM_TABLES, links, nullptr, n_links, w.stream, found.table, found.link)))
    return r;
  for (int t = 0; t < BP_NUM_TABLES; t++) {
    bp_witness_table& o = out->table[t];
    if (!tables[t].trace) continue;
    o.checked = 1;
    o.given = given_table(wit, tcfg, t);
    o.n_violated_rows = found.table[t].n_violated_rows;
    o.n_viol = found.table[t].n_viol;
    std::memcpy(o.viol, found.table[t].viol, sizeof(o.viol));
  }
  for (bp_witness_lookup& o : out->lookup) o.first_looking_row = o.first_looked_row = -1;
  for (uint32_t k = 0; k < n_links; k++) {
    bp_witness_lookup& o = out->lookup[pair[k]];
    const bp_set_link_report& f = found.link[k];
    o.checked = 1;
    o.holds = f.holds;
    o.n_looking = f.n_looking;
    o.n_looked = f.n_looked;
    o.first_looking_row = f.first_looking_row;
    o.first_looked_row = f.first_looked_row;
  }
  for (int t = 0; t < BP_NUM_TABLES; t++) {
    const bp_witness_table& o = out->table[t];
    if (o.given && o.n_violated_rows)
      return fail(BP_ERR_VERIFY, "the witness data given for table %s does not satisfy its AIR: row %u violates constraint %u "
                  "(family %u), %llu rows in all", TABLES[t].name, o.viol[0].row, o.viol[0].constraint, o.viol[0].family,
                  (unsigned long long)o.n_violated_rows);
  }
  for (uint32_t i = 0; i < air::ctl::N_PAIRS; i++) {
    const air::ctl::Pair& p = air::ctl::pairs()[i];
    const bp_witness_lookup& o = out->lookup[i];
    if (o.checked && !o.holds)
      return fail(BP_ERR_VERIFY, "cross-table lookup %s does not hold: first unmatched looking row %lld (table %s), looked row "
                  "%lld (table %s)", p.name, (long long)o.first_looking_row, TABLES[p.looking_table].name, (long long)o.first_looked_row,
                  TABLES[p.looked_table].name);
  }
  return BP_OK;
}
int bp_check_txn_witness(const bp_state* s, const uint8_t* ir, size_t ir_len, const bp_txn_witness* data, bp_witness_report* out) try {
  TxnWitness wit;
  if (int r = witness_of(data, &wit)) return r;
  return check_txn_impl(s, ir, ir_len, &wit, out);
}
BPG_ABI_CATCH("bp_check_txn_witness")
int bp_check_txn_witness_keccak(const bp_state* s, const uint8_t* ir, size_t ir_len, const uint64_t* keccak_inputs, size_t n_perms,
                                bp_witness_report* out) try {
  if (!keccak_inputs && n_perms) return fail(BP_ERR_INVALID_INPUT, "bp_check_txn_witness_keccak: null inputs");
  TxnWitness wit;
  wit.give(T_KECCAK, keccak_inputs, n_perms);
  return check_txn_impl(s, ir, ir_len, &wit, out);
}
BPG_ABI_CATCH("bp_check_txn_witness_keccak")

// What upstream's `prove` yields before the recursion (AllProof): the seven table proofs of a transaction on their one
// transcript, with the public values and the lookup challenges.  data as for bp_generate_txn_proof_witness (nullable).
int bp_generate_txn_table_proofs(const bp_state* s, const uint8_t* ir, size_t ir_len, const bp_txn_witness* data,
                                 const volatile uint8_t* abort_flag, uint8_t** out, size_t* out_len) try {
  TxnWitness wit;
  if (int r = witness_of(data, &wit)) return r;
  return txn_proof_of_one(s, ir, ir_len, &wit, nullptr, abort_flag, true, out, out_len);
}
BPG_ABI_CATCH("bp_generate_txn_table_proofs")
// The same for n transactions, table t of those whose shapes agree proved in lock-step (Tune::txn_group is not read: the
// caller has formed the group).  One group lease at a time: as many transactions as it grants, then the next ones.
// data: nullable, and so is every data[i].  outs[i] are the blobs bp_generate_txn_table_proofs gives, byte for byte; on
// a failure nothing is handed out.
int bp_generate_txn_table_proofs_group(const bp_state* s, const uint8_t* irs, size_t ir_stride, uint32_t n, const bp_txn_witness* const* data,
                                       const volatile uint8_t* abort_flag, uint8_t** outs, size_t* out_lens) try {
  if (!s || !irs || !outs || !out_lens || !n) return fail(BP_ERR_INVALID_INPUT, "bp_generate_txn_table_proofs_group: null argument");
  if (ir_stride < BP_IR_WORDS * 8) return fail(BP_ERR_INVALID_INPUT, "bp_generate_txn_table_proofs_group: ir_stride below %d bytes", BP_IR_WORDS * 8);
  std::vector<TxnWitness> wit(n);
  std::vector<const TxnWitness*> wp(n);
  std::vector<const uint8_t*> ip(n);
  for (uint32_t i = 0; i < n; i++) {
    if (int r = witness_of(data ? data[i] : nullptr, &wit[i])) return r;
    wp[i] = &wit[i];
    ip[i] = irs + (size_t)i * ir_stride;
    outs[i] = nullptr;
    out_lens[i] = 0;
  }
  for (uint32_t done = 0; done < n;) {
    uint32_t g = 0;
    if (int r = txn_proofs_impl(s, n - done, ip.data() + done, BP_IR_WORDS * 8, wp.data() + done, nullptr, abort_flag, true, nullptr, nullptr, nullptr,
                               outs + done, out_lens + done, &g)) {
      for (uint32_t i = 0; i < n; i++) { std::free(outs[i]); outs[i] = nullptr; out_lens[i] = 0; }
      return r;
    }
    done += g;
  }
  return BP_OK;
}
BPG_ABI_CATCH("bp_generate_txn_table_proofs_group")

// The host half of an aggregation: the children parsed, checked for contiguity and verified (or recognised as this
// state's own), the public-input list and the two path witnesses of the aggregation circuit.  No device work.
static int agg_prepare(const bp_state* s, const uint8_t* lhs, size_t lhs_len, int lhs_is_agg, const uint8_t* rhs, size_t rhs_len,
                       int rhs_is_agg, std::vector<uint64_t>* pi_out, std::vector<PathWitness>* paths_out) {
  if (!s || !lhs || !rhs) return fail(BP_ERR_INVALID_INPUT, "bp_generate_agg_proof: null argument");
  Box L, R;
  int r;
  if ((r = parse_box(lhs, lhs_len, s->rec_cfg, &L)) || (r = parse_box(rhs, rhs_len, s->rec_cfg, &R))) return r;
  if ((L.kind == 1) != (lhs_is_agg != 0) || (R.kind == 1) != (rhs_is_agg != 0) || L.kind > 1 || R.kind > 1)
    return fail(BP_ERR_INVALID_INPUT, "is_agg flags do not match the child proofs");
  // children must cover contiguous txn ranges (proof_types.rs:23-24)
  if (L.pv[1] != R.pv[0]) return fail(BP_ERR_INVALID_INPUT, "children are not contiguous: lhs ends at txn %llu, rhs starts at %llu",
                                      (unsigned long long)L.pv[1], (unsigned long long)R.pv[0]);
  if (L.pv[3] != R.pv[2] || std::memcmp(L.pv + 8, R.pv + 4, 32) != 0 || L.pv[12] != R.pv[12])
    return fail(BP_ERR_INVALID_INPUT, "children public values do not chain (gas / state root / block number)");
  {
    // A child this state produced is recognised by its hash and costs one Keccak; only two FOREIGN children (the
    // sub-block proofs gathered from other ranks, 10 ms of host Poseidon each) are verified side by side.  The
    // helper's message is thread-local, so it is carried over; the guard joins on every way out of the scope, so
    // an exception on this thread cannot reach a joinable std::thread's destructor (std::terminate).
    const bool l_known = produced_here(s, lhs, lhs_len), r_known = produced_here(s, rhs, rhs_len);
    int r_rhs = BP_OK;
    std::string lhs_err, rhs_err;
    std::thread helper;
    struct Joiner {
      std::thread& t;
      ~Joiner() { if (t.joinable()) t.join(); }
    } joiner{helper};
    bool rhs_done = r_known;
    if (!l_known && !r_known) {
      try {
        helper = std::thread([&] {
          try {
            r_rhs = verify_foreign(s, R, "rhs child proof");
            if (r_rhs) rhs_err = bp_last_error();
          } catch (...) {
            r_rhs = BP_ERR_DEVICE;
            rhs_err = "rhs child proof: out of memory while verifying";
          }
        });
        rhs_done = true;
      } catch (const std::system_error&) {  // no thread to be had: verify in this one
      }
    }
    r = l_known ? BP_OK : verify_foreign(s, L, "lhs child proof");
    if (r) lhs_err = bp_last_error();
    if (helper.joinable()) helper.join();
    if (!rhs_done && (r_rhs = verify_foreign(s, R, "rhs child proof"))) rhs_err = bp_last_error();
    if (r) return fail(r, "%s", lhs_err.c_str());
    if (r_rhs) return fail(r_rhs, "%s", rhs_err.c_str());
  }
  std::vector<uint64_t>& pi = *pi_out;
  pi.assign(AGG_PATH_PI0 + 16 + BP_PV_WORDS, 0);
  proof_digest(s->rec_cfg, L.stark, &pi[0]);
  proof_digest(s->rec_cfg, R.stark, &pi[4]);
  pi[8] = lhs_is_agg != 0; pi[9] = rhs_is_agg != 0;
  // per child the opened trace row of its first query and the cap entry above it: the circuit walks the path between them
  std::vector<PathWitness>& paths = *paths_out;
  paths.assign(2, PathWitness());
  first_query_trace_path(s->rec_cfg, L.stark, &pi[AGG_PATH_PI0], &pi[AGG_PATH_PI0 + 4], &paths[0]);
  first_query_trace_path(s->rec_cfg, R.stark, &pi[AGG_PATH_PI0 + 8], &pi[AGG_PATH_PI0 + 12], &paths[1]);
  uint64_t* pv = &pi[AGG_PATH_PI0 + 16];
  pv[0] = L.pv[0]; pv[1] = R.pv[1]; pv[2] = L.pv[2]; pv[3] = R.pv[3];
  std::memcpy(pv + 4, L.pv + 4, 32); std::memcpy(pv + 8, R.pv + 8, 32);
  pv[12] = L.pv[12];
  return BP_OK;
}

int bp_generate_agg_proof(const bp_state* s, const uint8_t* lhs, size_t lhs_len, int lhs_is_agg,
                          const uint8_t* rhs, size_t rhs_len, int rhs_is_agg, uint8_t** out, size_t* out_len) try {
  if (!s || !lhs || !rhs || !out || !out_len) return fail(BP_ERR_INVALID_INPUT, "bp_generate_agg_proof: null argument");
  std::vector<uint64_t> pi;
  std::vector<PathWitness> paths;
  int r = agg_prepare(s, lhs, lhs_len, lhs_is_agg, rhs, rhs_len, rhs_is_agg, &pi, &paths);
  if (r) return r;
  (void)hipSetDevice(s->cfg.device);
  ProverLease lease(s);
  std::vector<uint64_t> proof;
  if ((r = rec_prove(*lease.w, s->rec_cfg, s->special[1], pi, proof, &paths))) return r;
  if ((r = emit_box(1, CIRCUIT_AGG, pi, proof, out, out_len))) return r;
  remember_proof(s, *out, *out_len);
  return BP_OK;
}
BPG_ABI_CATCH("bp_generate_agg_proof")

int bp_generate_block_proof(const bp_state* s, const uint8_t* parent, size_t parent_len, const uint8_t* agg,
                            size_t agg_len, uint8_t** out, size_t* out_len, uint64_t* b_height) try {
  if (!s || !agg || !out || !out_len) return fail(BP_ERR_INVALID_INPUT, "bp_generate_block_proof: null argument");
  Box A, Pb;
  int r;
  if ((r = parse_box(agg, agg_len, s->rec_cfg, &A))) return r;
  if (A.kind != 1) return fail(BP_ERR_INVALID_INPUT, "curr_block_agg_proof is not an aggregation proof");
  std::vector<uint64_t> pi(BLOCK_PATH_PI0 + 8 + BP_PV_WORDS, 0);
  if (parent) {
    if ((r = parse_box(parent, parent_len, s->rec_cfg, &Pb))) return r;
    if (Pb.kind != 2) return fail(BP_ERR_INVALID_INPUT, "parent is not a block proof");
    if (Pb.pv[12] + 1 != A.pv[12]) return fail(BP_ERR_INVALID_INPUT, "parent block height %llu does not precede %llu",
                                                (unsigned long long)Pb.pv[12], (unsigned long long)A.pv[12]);
    if ((r = verify_child(s, Pb, "parent block proof", parent, parent_len))) return r;
    proof_digest(s->rec_cfg, Pb.stark, &pi[0]);
    pi[8] = 1;
  }
  if ((r = verify_child(s, A, "curr_block_agg_proof", agg, agg_len))) return r;
  proof_digest(s->rec_cfg, A.stark, &pi[4]);
  std::vector<PathWitness> paths(1);
  first_query_trace_path(s->rec_cfg, A.stark, &pi[BLOCK_PATH_PI0], &pi[BLOCK_PATH_PI0 + 4], &paths[0]);
  std::memcpy(&pi[BLOCK_PATH_PI0 + 8], A.pv, BP_PV_WORDS * 8);
  (void)hipSetDevice(s->cfg.device);
  ProverLease lease(s);
  std::vector<uint64_t> proof;
  if ((r = rec_prove(*lease.w, s->rec_cfg, s->special[2], pi, proof, &paths))) return r;
  if (b_height) *b_height = A.pv[12];  // block_metadata.block_number.low_u64(), proof_gen.rs:90-94
  if ((r = emit_box(2, CIRCUIT_BLOCK, pi, proof, out, out_len))) return r;
  remember_proof(s, *out, *out_len);
  return BP_OK;
}
BPG_ABI_CATCH("bp_generate_block_proof")

int bp_verifier_state_from_prover(const bp_state* s, bp_verifier_state** out) try {
  if (!s || !out) return fail(BP_ERR_INVALID_INPUT, "bp_verifier_state_from_prover: null argument");
  bp_verifier_state* v = new bp_verifier_state();
  v->rec_cfg = s->rec_cfg;
  for (int k = 0; k < 3; k++) {
    v->special[k].cap = s->special[k].consts.cap;
    std::memcpy(v->special[k].digest, s->special[k].digest, 32);
  }
  *out = v;
  return BP_OK;
}
BPG_ABI_CATCH("bp_verifier_state_from_prover")
// ProverStateBuilder::build_verifier (verifier_state.rs:34-42): build the circuits, keep the light part.
int bp_verifier_state_build(const bp_config* cfg, bp_verifier_state** out) try {
  bp_state* s = nullptr;
  bp_config c = *cfg;
  c.n_workers = 1;
  int r = bp_state_build(&c, &s);
  if (r) return r;
  r = bp_verifier_state_from_prover(s, out);
  bp_state_free(s);
  return r;
}
BPG_ABI_CATCH("bp_verifier_state_build")
// Light verifier data from raw caps (what a verifier-only deployment would load from disk):
// caps = root, agg, block constants caps, each 4 << stark_cap_height words.  CPU only.
int bp_verifier_state_from_caps(const bp_config* cfg, const uint64_t* caps, bp_verifier_state** out) try {
  if (!cfg || !caps || !out) return fail(BP_ERR_INVALID_INPUT, "bp_verifier_state_from_caps: null argument");
  const StarkCfg rc = rec_cfg_of(*cfg);
  int r = check_cfg(rc);
  if (r) return r;
  const size_t cw = (size_t)4 << rc.cap_height;
  for (size_t i = 0; i < 3 * cw; i++) if (caps[i] >= gl::P) return fail(BP_ERR_INVALID_INPUT, "non-canonical cap word");
  bp_verifier_state* v = new bp_verifier_state();
  v->rec_cfg = rc;
  for (int k = 0; k < 3; k++) {
    v->special[k].cap.assign(caps + k * cw, caps + (k + 1) * cw);
    hash_no_pad_host(v->special[k].cap.data(), cw, v->special[k].digest);
  }
  *out = v;
  return BP_OK;
}
BPG_ABI_CATCH("bp_verifier_state_from_caps")
void bp_verifier_state_free(bp_verifier_state* v) { delete v; }

int bp_verify_proof(const bp_verifier_state* v, const uint8_t* proof, size_t len) try {
  if (!v || !proof) return fail(BP_ERR_INVALID_INPUT, "bp_verify_proof: null argument");
  Box b;
  int r = parse_box(proof, len, v->rec_cfg, &b);
  if (r) return r;
  if (b.circuit != CIRCUIT_ROOT + b.kind) return fail(BP_ERR_VERIFY, "proof was made by circuit %llu, expected %u",
                                                      (unsigned long long)b.circuit, CIRCUIT_ROOT + (uint32_t)b.kind);
  for (size_t i = 0; i < b.n_pi; i++) if (b.pi[i] >= gl::P) return fail(BP_ERR_VERIFY, "non-canonical public input");
  return rec_verify(v->rec_cfg, v->special[b.kind], b);
}
BPG_ABI_CATCH("bp_verify_proof")
int bp_verify_block_proof(const bp_verifier_state* v, const uint8_t* proof, size_t len) try {
  if (!v || !proof) return fail(BP_ERR_INVALID_INPUT, "bp_verify_block_proof: null argument");
  Box b;
  int r = parse_box(proof, len, v->rec_cfg, &b);
  if (r) return r;
  if (b.kind != 2) return fail(BP_ERR_VERIFY, "not a block proof");
  return bp_verify_proof(v, proof, len);
}
BPG_ABI_CATCH("bp_verify_block_proof")

}  // extern "C"

// ---- the prover's side of a shard's job pool (rec_pool.hpp; the scheduler is gi.cpp's) ------------------------------
namespace bpg {

uint32_t rec_batch_cap(const bp_state* s) { return s ? batch_cap(s->rec_cfg) : 1; }

uint32_t state_workers(const bp_state* s) { return s ? s->cfg.n_workers : 1; }
uint32_t txn_group_of(const bp_state* s) {
  const int knob = tune().txn_group.load(std::memory_order_relaxed);
  return knob > 0 ? (uint32_t)knob : (s ? s->auto_txn_group : 1);
}

int txn_group_pooled(const bp_state* s, uint32_t n, const uint8_t* const* irs, size_t ir_len, const bp_txn_witness* const* data,
                     const volatile uint8_t* abort_flag, RecPool* pool, const uint32_t* nodes, const std::function<void(uint32_t)>& granted,
                     TreeBuf* outs) {
  if (!n || n > MAX_BATCH || !nodes || (!pool && !outs)) return fail(BP_ERR_INVALID_INPUT, "txn_group_pooled: a group of %u", n);
  TxnWitness wit[MAX_BATCH];
  const TxnWitness* wp[MAX_BATCH];
  for (uint32_t i = 0; i < n; i++) {
    if (int r = witness_of(data ? data[i] : nullptr, &wit[i])) return r;
    wp[i] = &wit[i];
  }
  uint8_t* o[MAX_BATCH] = {};
  size_t ol[MAX_BATCH] = {};
  const int r = txn_proofs_impl(s, n, irs, ir_len, wp, nullptr, abort_flag, false, pool, nodes, &granted, pool ? nullptr : o, pool ? nullptr : ol, nullptr);
  for (uint32_t i = 0; i < n && !pool; i++) {
    if (r) std::free(o[i]);
    else outs[i] = TreeBuf{o[i], ol[i]};
  }
  return r;
}

int agg_proof_prepare(const bp_state* s, const uint8_t* lhs, size_t lhs_len, int lhs_is_agg, const uint8_t* rhs, size_t rhs_len,
                      int rhs_is_agg, RecJob* job) {
  if (!job) return fail(BP_ERR_INVALID_INPUT, "agg_proof_prepare: no job");
  if (int r = agg_prepare(s, lhs, lhs_len, lhs_is_agg, rhs, rhs_len, rhs_is_agg, &job->pi, &job->paths)) return r;
  job->kind = 1;
  job->circuit = &s->special[1];
  return BP_OK;
}

int rec_prove_jobs(const bp_state* s, const std::vector<std::unique_ptr<RecJob>>& jobs, const volatile uint8_t* abort_flag,
                   std::vector<TreeBuf>* out) {
  if (!s || !out || jobs.empty()) return fail(BP_ERR_INVALID_INPUT, "rec_prove_jobs: nothing to prove");
  const size_t n = jobs.size();
  std::vector<const Circuit*> circ(n);
  std::vector<std::vector<uint64_t>> pi(n), proofs(n);
  std::vector<std::vector<PathWitness>> paths(n);
  for (size_t k = 0; k < n; k++) {
    circ[k] = static_cast<const Circuit*>(jobs[k]->circuit);
    pi[k] = jobs[k]->pi;
    paths[k] = jobs[k]->paths;
  }
  (void)hipSetDevice(s->cfg.device);
  {
    ProverLease lease(s);
    Worker& w = *lease.w;
    w.abort_flag_u8 = abort_flag;
    if (w.aborted()) return fail(BP_ERR_ABORTED, "aborted before a batch of %zu recursion jobs", n);
    if (int r = rec_prove_batch(w, s->rec_cfg, (uint32_t)n, circ.data(), pi.data(), proofs.data(), paths.data())) return r;
  }
  out->assign(n, TreeBuf());
  for (size_t k = 0; k < n; k++)
    if (int r = box_of_job(s, *jobs[k], proofs[k], &(*out)[k])) {
      for (auto& b : *out) std::free(b.p);
      out->clear();
      return r;
    }
  return BP_OK;
}

}  // namespace bpg
