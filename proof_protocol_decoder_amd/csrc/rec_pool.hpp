// rec_pool.hpp -- recursion-shaped proofs as JOBS, and the shard scheduler that feeds on them (gi.cpp, proofgen.cpp).
//
// A transaction's three lock-step batches hold seven proofs each and a batch has room for eight (MAX_BATCH): the root
// proof of a transaction and the aggregation proofs of the tree are proofs of the same shape whose inputs are host data,
// so any prover can carry one of them as the eighth slot of a batch it launches anyway.  A chain of one costs the same
// ~57 launches and host round trips as a chain of seven; riding, it costs none.  A group of g transactions proves a level
// of all its chains as one batch (proofgen.cpp: group_recursion, Tune::rec_group): 7 g proofs, and the slots a batch of
// MAX_LOCKSTEP = 24 leaves free -- three at g = 3 -- carry riders the same way.
//
//  * RecJob: one such proof to be made -- circuit, public-input list, path witnesses -- and the tree node it is for.
//  * RecPool: post a job, take up to k ready jobs (aggregations before roots, each in node order), hand back the
//    finished container (complete) or a failure (fail).
//  * TreeRun: the scheduler of a contiguous slice and its aggregation tree.  Leaves go to the threads in order; an
//    aggregation whose children exist goes AHEAD of the leaves still waiting (its host preparation, then a job); a
//    thread that finds nothing to start while jobs are ready proves up to a batch of them.  A thread never waits for a
//    rider.  The first failure -- of a leaf, a preparation, a batch or a rider -- stops the pool; its status and message
//    are the call's.
//
// Plain C++: no HIP, no prover types (a circuit is an opaque pointer), so tools/rec_pool_check.cpp builds it alone
// under the thread and address sanitizers with fake leaves and batches.
#pragma once
#include <algorithm>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <queue>
#include <string>
#include <system_error>
#include <thread>
#include <utility>
#include <vector>
#include "../../include/bpg.h"

namespace bpg {

// One Merkle path a recursion circuit walks in its Poseidon rows: the leaf digest and the cap entry are words of the
// proof's public-input list (Layout::path_pi0), the position and the siblings are witness.
struct PathWitness {
  uint64_t index = 0;
  std::vector<uint64_t> siblings;  // 4 words per level, leaf upward
  std::vector<uint64_t> leaf_row;  // the opened row the leaf digest is the hash of (circuits that hash it: Layout::leaf_len)
};

struct RecJob {
  uint32_t node = 0;                // the tree node the finished container is the result of
  uint32_t kind = 0;                // container kind: 0 = a transaction's root proof, 1 = an aggregation proof
  const void* circuit = nullptr;    // the prover's preprocessed circuit (proofgen.cpp: Circuit)
  std::vector<uint64_t> pi;         // the public-input list the container carries and the circuit hashes
  std::vector<PathWitness> paths;   // one per Merkle path the circuit walks
};

struct TreeBuf {  // a malloc'ed proof container
  uint8_t* p = nullptr;
  size_t n = 0;
};

class RecPool {
 public:
  virtual ~RecPool() = default;
  RecPool() = default;
  RecPool(const RecPool&) = delete;
  RecPool& operator=(const RecPool&) = delete;

  // the job is ready to be proved by whoever has a slot for it
  void post(std::unique_ptr<RecJob> job) noexcept {
    std::lock_guard<std::mutex> lk(mu_);
    try {
      const std::pair<int, uint32_t> key{job->kind == 1 ? 0 : 1, job->node};
      ready_.emplace(key, std::move(job));
    } catch (...) {
      fail_locked(BP_ERR_DEVICE, "out of memory while posting a recursion job");
    }
    cv_.notify_all();
  }
  // up to k ready jobs, appended to *out; none once the pool has stopped
  size_t take(size_t k, std::vector<std::unique_ptr<RecJob>>* out) noexcept {
    std::lock_guard<std::mutex> lk(mu_);
    return take_locked(k, out);
  }
  // the finished container of a job that was taken; the bytes are the pool's from here on
  void complete(const RecJob& job, uint8_t* bytes, size_t len) noexcept {
    std::lock_guard<std::mutex> lk(mu_);
    node_done_guarded(job.node, bytes, len);
  }
  // the first failure is the pool's status; every failure stops it
  void fail(int status, const char* msg) noexcept {
    std::lock_guard<std::mutex> lk(mu_);
    fail_locked(status, msg);
  }

 protected:
  virtual void node_done_locked(uint32_t node, uint8_t* bytes, size_t len) = 0;  // mu_ held; takes the bytes first
  void node_done_guarded(uint32_t node, uint8_t* bytes, size_t len) noexcept {
    try {
      node_done_locked(node, bytes, len);
    } catch (...) {  // the bookkeeping allocates (the queue of nodes to start): no exception leaves a thread
      fail_locked(BP_ERR_DEVICE, "out of memory in the shard's bookkeeping");
    }
    cv_.notify_all();
  }
  size_t take_locked(size_t k, std::vector<std::unique_ptr<RecJob>>* out) noexcept {
    size_t got = 0;
    if (stop_) return 0;
    try {
      out->reserve(out->size() + std::min(k, ready_.size()));
      while (got < k && !ready_.empty()) {
        out->push_back(std::move(ready_.begin()->second));
        ready_.erase(ready_.begin());
        got++;
      }
    } catch (...) {
      fail_locked(BP_ERR_DEVICE, "out of memory while taking recursion jobs");
    }
    return got;
  }
  void fail_locked(int status, const char* msg) noexcept {
    if (!first_rc_) {
      first_rc_ = status ? status : (int)BP_ERR_DEVICE;
      try {
        first_msg_ = msg ? msg : "";
      } catch (...) {
      }
    }
    stop_ = true;
    cv_.notify_all();
  }

  std::mutex mu_;
  std::condition_variable cv_;
  bool stop_ = false;
  int first_rc_ = BP_OK;
  std::string first_msg_;
  std::map<std::pair<int, uint32_t>, std::unique_ptr<RecJob>> ready_;  // (0 aggregation / 1 root, node) -> job
};

// Entry k of the plan is node n + k = (left, right) node ids; the last entry is the root.  Aggregation needs contiguous
// ranges (proof_types.rs:23-24) and nothing else.  0 = balanced: adjacent pairs level by level, an odd tail carried up;
// 1 = pairs_then_chain: adjacent leaves paired, the pair results folded left to right.  false: n = 0 or an unknown shape.
inline bool tree_plan(uint32_t n, uint32_t shape, std::vector<std::pair<uint32_t, uint32_t>>* plan) {
  plan->clear();
  if (n < 1 || shape > 1) return false;
  if (shape == 0) {
    std::vector<uint32_t> level(n);
    for (uint32_t i = 0; i < n; i++) level[i] = i;
    while (level.size() > 1) {
      std::vector<uint32_t> nxt;
      for (size_t k = 0; k + 1 < level.size(); k += 2) {
        plan->push_back({level[k], level[k + 1]});
        nxt.push_back(n + (uint32_t)plan->size() - 1);
      }
      if (level.size() % 2) nxt.push_back(level.back());
      level.swap(nxt);
    }
    return true;
  }
  std::vector<uint32_t> heads;
  for (uint32_t k = 0; k + 1 < n; k += 2) {
    plan->push_back({k, k + 1});
    heads.push_back(n + (uint32_t)plan->size() - 1);
  }
  if (n % 2) heads.push_back(n - 1);
  uint32_t acc = heads[0];
  for (size_t i = 1; i < heads.size(); i++) {
    plan->push_back({acc, heads[i]});
    acc = n + (uint32_t)plan->size() - 1;
  }
  return true;
}

// What the scheduler calls.  Every callback returns a bp_status; after a failure last_error() is its message.
struct TreeOps {
  // Leaf i.  Either its container comes back in *out (malloc'ed), or -- pool given -- the leaf has posted the job that
  // makes it (node i) and says so in *posted.  pool is null when the run carries no jobs.
  std::function<int(uint32_t i, RecPool* pool, uint8_t** out, size_t* out_len, bool* posted)> leaf;
  // An aggregation proved on the spot (a run without jobs).
  std::function<int(const TreeBuf& l, int l_agg, const TreeBuf& r, int r_agg, uint8_t** out, size_t* out_len)> agg;
  // The host half of an aggregation: children parsed and checked, job->kind / circuit / pi / paths filled.
  std::function<int(const TreeBuf& l, int l_agg, const TreeBuf& r, int r_agg, RecJob* job)> agg_prepare;
  // Up to `cap` jobs proved as one lock-step batch: (*out)[k] is the container of jobs[k].
  std::function<int(const std::vector<std::unique_ptr<RecJob>>& jobs, std::vector<TreeBuf>* out)> prove_batch;
  std::function<std::string()> last_error;
  uint32_t cap = 1;     // jobs a drained batch holds
  bool pooled = false;  // roots and aggregations are jobs (else every node is proved where it is started)
  // Leaves ids[0..n) (ascending) started by ONE thread as a group (Tune::txn_group).  The callee may take fewer than it
  // is offered: it calls granted(g), 1 <= g <= n, once and as soon as it knows -- the leaves ids[g..n) then go back to
  // the queue at once, for other threads -- and starts ids[0..g): per leaf a container in outs[k], or with a pool the
  // job posted.  A callee that returns without having called it has taken all n.
  std::function<int(const uint32_t* ids, uint32_t n, RecPool* pool, const std::function<void(uint32_t)>& granted, TreeBuf* outs)> leaf_group;
  uint32_t group = 1;   // leaves a thread may start at a time (1, or no leaf_group: one leaf per thread as ever)
  uint32_t lanes = 0;   // provers the leaves' callee can lease at a time (a state's n_workers); read when group > 1
};

class TreeRun : public RecPool {
 public:
  // leaf_is_agg (nullable): the kinds of the leaves when they are proofs made elsewhere; else txn proofs.
  // keep_leaves: the caller wants the leaves' containers, so an aggregation does not free them.
  TreeRun(uint32_t n, std::vector<std::pair<uint32_t, uint32_t>> plan, const TreeOps& ops, const volatile uint8_t* abort_flag,
          const int* leaf_is_agg, bool keep_leaves)
      : n_(n), plan_(std::move(plan)), ops_(ops), abort_flag_(abort_flag), leaf_is_agg_(leaf_is_agg), keep_leaves_(keep_leaves) {
    total_ = n_ + (uint32_t)plan_.size();
    root_ = total_ - 1;
    parent_of_.assign(total_, ~0u);
    for (uint32_t k = 0; k < plan_.size(); k++) parent_of_[plan_[k].first] = parent_of_[plan_[k].second] = n_ + k;
    res_.resize(total_);
    done_.assign(total_, 0);
    for (uint32_t i = 0; i < n_; i++) queue_.push({1, i});
  }
  ~TreeRun() override {
    for (auto& b : res_) std::free(b.p);
  }
  // Runs the tree on n_threads threads (the caller's is one of them); all of them have been joined on return.
  int run(uint32_t n_threads) {
    n_threads = std::min<uint32_t>(std::min<uint32_t>(n_threads ? n_threads : 1, n_), 256);
    n_threads_ = n_threads;
    std::vector<std::thread> pool;
    struct Joiner {
      std::vector<std::thread>& p;
      ~Joiner() { for (auto& t : p) if (t.joinable()) t.join(); }
    } joiner{pool};
    try {
      pool.reserve(n_threads);
      for (uint32_t i = 1; i < n_threads; i++) pool.emplace_back([this] { worker(); });
    } catch (const std::system_error&) {  // no more threads to be had: the ones there are do the work
    } catch (const std::bad_alloc&) {
    }
    worker();  // the calling thread is one of the pool
    for (auto& t : pool) t.join();
    pool.clear();
    return first_rc_;
  }
  const std::string& error() const { return first_msg_; }
  uint32_t root() const { return root_; }
  const TreeBuf& result(uint32_t node) const { return res_[node]; }
  TreeBuf release(uint32_t node) {  // the container becomes the caller's
    TreeBuf b = res_[node];
    res_[node] = TreeBuf();
    return b;
  }

 protected:
  void node_done_locked(uint32_t nid, uint8_t* bytes, size_t len) override {
    if (nid >= total_ || done_[nid]) {
      std::free(bytes);
      fail_locked(BP_ERR_DEVICE, "a node of the shard was completed twice");
      return;
    }
    res_[nid] = TreeBuf{bytes, len};
    done_[nid] = 1;
    if (nid >= n_) {  // the children have been consumed: leaves stay when the caller wants them
      const uint32_t ch[2] = {plan_[nid - n_].first, plan_[nid - n_].second};
      for (uint32_t c : ch)
        if (c >= n_ || !keep_leaves_) { std::free(res_[c].p); res_[c] = TreeBuf(); }
    }
    const uint32_t par = parent_of_[nid];
    if (par != ~0u && done_[plan_[par - n_].first] && done_[plan_[par - n_].second]) queue_.push({0, par});
    if (nid == root_) stop_ = true;
  }

 private:
  // (the flag is the caller's AtomicBool, raised from another thread while the run is under way: an atomic load)
  bool aborted() const { return abort_flag_ && __atomic_load_n(abort_flag_, __ATOMIC_RELAXED); }
  void fail_with(int rc, const std::string& own) noexcept {
    try {
      const std::string msg = !own.empty() ? own : (ops_.last_error ? ops_.last_error() : std::string());
      fail(rc, msg.c_str());
    } catch (...) {
      fail(rc, "");
    }
  }
  static std::string text(const char* fmt, uint32_t v) {
    char buf[96];
    std::snprintf(buf, sizeof(buf), fmt, v);
    return buf;
  }
  // Groups (ops_.group > 1).  A thread that would start a leaf starts up to `group` of them as one call of leaf_group.
  // Every transaction of a group occupies one of the callee's `lanes` provers, so a thread takes leaves only while a
  // lane is free (it waits here, where it can still prepare aggregations, and not inside the callee's lease), and it
  // takes  min(group, free lanes, ceil(waiting leaves / threads that are not busy))  of them: while the shard is long
  // that is `group`; over the last round it falls to 1, so that the tail spreads over all the provers' streams instead
  // of leaving half of them idle behind a few groups.
  bool grouped() const { return ops_.group > 1 && ops_.leaf_group && ops_.lanes > 0; }
  bool leaf_startable() const { return !grouped() || lanes_used_ < ops_.lanes; }
  bool runnable() const {
    if (!queue_.empty()) return queue_.top().first == 0 || leaf_startable();
    return !ready_.empty();
  }
  void worker() noexcept {
    for (;;) {
      bool have = false;
      uint32_t nid = 0, n_group = 0, lanes_held = 0;
      uint32_t ids[kMaxGroup];
      std::vector<std::unique_ptr<RecJob>> batch;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return stop_ || runnable(); });
        if (stop_) return;
        if (!queue_.empty()) {  // an aggregation to prepare (or prove), else the next leaf
          nid = queue_.top().second;
          queue_.pop();
          have = true;
          if (nid < n_ && grouped()) {  // (the aggregations go first: what is left in the queue are leaves)
            const uint32_t waiting = (uint32_t)queue_.size() + 1, idle_threads = std::max<uint32_t>(1, n_threads_ - std::min(busy_, n_threads_ - 1));
            const uint32_t want = std::min(std::min<uint32_t>(std::min<uint32_t>(ops_.group, kMaxGroup), ops_.lanes - lanes_used_),
                                           (waiting + idle_threads - 1) / idle_threads);
            ids[n_group++] = nid;
            while (n_group < want && !queue_.empty() && queue_.top().first == 1) {
              ids[n_group++] = queue_.top().second;
              queue_.pop();
            }
            lanes_used_ += lanes_held = n_group;
          }
          busy_++;
        } else if (take_locked(ops_.cap ? ops_.cap : 1, &batch) == 0) {
          return;  // (only a failure inside take_locked: the pool has stopped)
        } else {
          busy_++;
        }
      }
      TreeBuf gouts[kMaxGroup];
      uint32_t n_taken = n_group;
      bool heard = false;
      // the callee has its lease: what it did not take goes back to the queue, in index order, and the lanes with it
      const std::function<void(uint32_t)> granted = [&](uint32_t g) {
        if (heard) return;
        heard = true;
        g = std::min(std::max<uint32_t>(g, 1), n_group);
        std::lock_guard<std::mutex> lk(mu_);
        try {
          for (uint32_t k = g; k < n_group; k++) queue_.push({1, ids[k]});
        } catch (...) {
          fail_locked(BP_ERR_DEVICE, "out of memory in the shard's bookkeeping");
        }
        lanes_used_ -= n_group - g;
        lanes_held = n_taken = g;
        cv_.notify_all();
      };
      // on every way out of this round: the thread is idle again, its lanes are free
      struct Round {
        TreeRun& t;
        uint32_t& lanes;
        ~Round() {
          std::lock_guard<std::mutex> lk(t.mu_);
          t.busy_--;
          t.lanes_used_ -= lanes;
          t.cv_.notify_all();
        }
      } round{*this, lanes_held};
      TreeBuf b;
      std::vector<TreeBuf> outs;
      int rc = BP_OK;
      std::string own;  // a message of the scheduler's own (else the callback's last_error)
      bool posted = false;
      try {
        if (aborted()) {
          rc = BP_ERR_ABORTED;
          own = have ? text("aborted before node %u of the shard", nid) : text("aborted before a batch of %u recursion jobs", (uint32_t)batch.size());
        } else if (!have) {
          rc = ops_.prove_batch(batch, &outs);
          if (rc == BP_OK && outs.size() != batch.size()) { rc = BP_ERR_DEVICE; own = "a batch of recursion jobs returned the wrong number of proofs"; }
          for (size_t k = 0; rc == BP_OK && k < outs.size(); k++)
            if (!outs[k].p) { rc = BP_ERR_DEVICE; own = text("node %u of the shard returned no proof", batch[k]->node); }
        } else if (n_group) {
          rc = ops_.leaf_group(ids, n_group, ops_.pooled ? this : nullptr, granted, gouts);
          posted = ops_.pooled;
          for (uint32_t k = 0; rc == BP_OK && !posted && k < n_taken; k++)
            if (!gouts[k].p) { rc = BP_ERR_DEVICE; own = text("node %u of the shard returned no proof", ids[k]); }
          if (rc == BP_OK && !posted) posted = true;  // (the containers are handed over below)
        } else if (nid < n_) {
          rc = ops_.leaf(nid, ops_.pooled ? this : nullptr, &b.p, &b.n, &posted);
        } else {
          const uint32_t l = plan_[nid - n_].first, r = plan_[nid - n_].second;
          const int la = l >= n_ || (leaf_is_agg_ && leaf_is_agg_[l]), ra = r >= n_ || (leaf_is_agg_ && leaf_is_agg_[r]);
          if (ops_.pooled) {
            std::unique_ptr<RecJob> job(new RecJob());
            job->node = nid;
            rc = ops_.agg_prepare(res_[l], la, res_[r], ra, job.get());
            if (rc == BP_OK) { post(std::move(job)); posted = true; }
          } else {
            rc = ops_.agg(res_[l], la, res_[r], ra, &b.p, &b.n);
          }
        }
        if (have && rc == BP_OK && !b.p && !posted) { rc = BP_ERR_DEVICE; own = text("node %u of the shard returned no proof", nid); }
      } catch (...) {
        rc = BP_ERR_DEVICE;
        own = have ? text("node %u of the shard: exception in a callback", nid) : "a batch of recursion jobs: exception in a callback";
      }
      if (rc) {
        std::free(b.p);
        for (auto& o : outs) std::free(o.p);
        for (auto& o : gouts) std::free(o.p);
        fail_with(rc, own);
        return;
      }
      if (!have) {
        for (size_t k = 0; k < batch.size(); k++) complete(*batch[k], outs[k].p, outs[k].n);
      } else if (n_group) {
        std::lock_guard<std::mutex> lk(mu_);
        for (uint32_t k = 0; k < n_taken; k++)
          if (gouts[k].p) node_done_guarded(ids[k], gouts[k].p, gouts[k].n);
      } else if (b.p) {
        std::lock_guard<std::mutex> lk(mu_);
        node_done_guarded(nid, b.p, b.n);
      }
    }
  }

  static constexpr uint32_t kMaxGroup = 8;  // (the prover's MAX_BATCH)
  uint32_t n_threads_ = 1, busy_ = 0, lanes_used_ = 0;  // under mu_
  const uint32_t n_;
  const std::vector<std::pair<uint32_t, uint32_t>> plan_;
  const TreeOps ops_;
  const volatile uint8_t* const abort_flag_;
  const int* const leaf_is_agg_;
  const bool keep_leaves_;
  uint32_t total_ = 0, root_ = 0;
  std::vector<uint32_t> parent_of_;
  std::vector<TreeBuf> res_;
  std::vector<char> done_;
  using Item = std::pair<int, uint32_t>;
  std::priority_queue<Item, std::vector<Item>, std::greater<Item>> queue_;  // 0 aggregation before 1 leaf, each in index order
};

}  // namespace bpg

// ---- the prover's side (proofgen.cpp), for the scheduler of a state-backed shard (gi.cpp) ----
namespace bpg {
// proofs one lock-step batch holds for this state's recursion shape (MAX_BATCH, Tune::rec_batch, the query limit)
uint32_t rec_batch_cap(const bp_state* s);
// the host half of bp_generate_agg_proof: everything but the proving
int agg_proof_prepare(const bp_state* s, const uint8_t* lhs, size_t lhs_len, int lhs_is_agg, const uint8_t* rhs, size_t rhs_len,
                      int rhs_is_agg, RecJob* job);
// bp_generate_txn_proof_witness for up to n <= MAX_BATCH transactions on one lease (proofgen.cpp: ProverLease,
// prove_tables; a lone transaction is a group of one): the first g the lease grants -- granted(g) is called when it is
// held.  With a pool the chain batches carry its ready jobs in their spare slots and the roots are posted as the jobs of
// nodes[i]; without one the containers land in outs[i].  data nullable, and every data[i].
int txn_group_pooled(const bp_state* s, uint32_t n, const uint8_t* const* irs, size_t ir_len, const bp_txn_witness* const* data,
                     const volatile uint8_t* abort_flag, RecPool* pool, const uint32_t* nodes, const std::function<void(uint32_t)>& granted,
                     TreeBuf* outs);
uint32_t state_workers(const bp_state* s);
uint32_t txn_group_of(const bp_state* s);  // Tune::txn_group, or what the state's queue count asks for (0 = automatic)
// the jobs proved in lock-step on one leased prover; (*out)[k] = the container of jobs[k], remembered as this state's own
int rec_prove_jobs(const bp_state* s, const std::vector<std::unique_ptr<RecJob>>& jobs, const volatile uint8_t* abort_flag,
                   std::vector<TreeBuf>* out);
}  // namespace bpg
