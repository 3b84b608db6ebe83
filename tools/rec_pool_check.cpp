// rec_pool_check.cpp -- the shard scheduler and its job pool (csrc/rec_pool.hpp) alone, with fake provers.
//
// No device, no library: leaves, aggregations and "batches" only record which jobs they carried.  A fake transaction
// does what txn_proof_impl does with the pool -- three batches of seven that each take up to cap - 7 riders and hand
// their containers back, then the root posted as a job -- and a fake container is the id of its node, so every check
// below reads what the scheduler did from the data it moved:
//   * every node is completed exactly once, and the root's container is the root's;
//   * no batch holds more than 8 proofs;
//   * an aggregation's preparation sees the containers of exactly its two children (so it never starts before them);
//   * a failing leaf or a failing rider ends the run with that status and message, with every thread joined.
// Cases: n in {1, 2, 3, 5, 8, 13, 32} x threads in {1, 2, 4} x both tree shapes, with and without jobs.
// Built by tests/test_rec_pool.py with -fsanitize=thread and, a second time, -fsanitize=address,undefined.
//   c++ -std=c++17 -O1 -g -pthread -fsanitize=thread tools/rec_pool_check.cpp -o rec_pool_check && ./rec_pool_check
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include "../proof_protocol_decoder_amd/csrc/rec_pool.hpp"

namespace {

constexpr uint32_t CAP = 8, HOSTS = 7;
thread_local std::string t_error;

int fail_with(int rc, const std::string& msg) {
  t_error = msg;
  return rc;
}
uint8_t* box_of(uint32_t node, size_t* len) {
  uint32_t* p = static_cast<uint32_t*>(std::malloc(sizeof(uint32_t)));
  *p = node;
  *len = sizeof(uint32_t);
  return reinterpret_cast<uint8_t*>(p);
}
uint32_t node_of(const bpg::TreeBuf& b) {
  uint32_t v = ~0u;
  if (b.p && b.n == sizeof(v)) std::memcpy(&v, b.p, sizeof(v));
  return v;
}

struct Case {
  uint32_t n, threads, shape;
  bool pooled, keep_leaves;
  int fail_leaf = -1;   // this leaf returns BP_ERR_RANGE
  int fail_job = -1;    // the batch that carries this node's job returns BP_ERR_VERIFY
};

struct Record {
  std::vector<std::atomic<int>> made;      // containers made per node
  std::atomic<int> max_batch{0}, in_callback{0}, bad{0}, rider_slots{0}, drained{0};
  explicit Record(size_t total) : made(total) {
    for (auto& m : made) m.store(0);
  }
  void batch(int size) {
    int cur = max_batch.load();
    while (size > cur && !max_batch.compare_exchange_weak(cur, size)) {
    }
  }
};
struct InCallback {
  Record& r;
  explicit InCallback(Record& rec) : r(rec) { r.in_callback++; }
  ~InCallback() { r.in_callback--; }
};

bool complain(const Case& c, const char* what) {
  std::printf("FAILED n=%u threads=%u shape=%u pooled=%d keep=%d fail_leaf=%d fail_job=%d: %s\n", c.n, c.threads, c.shape, (int)c.pooled,
              (int)c.keep_leaves, c.fail_leaf, c.fail_job, what);
  return false;
}

bool run_case(const Case& c) {
  std::vector<std::pair<uint32_t, uint32_t>> plan;
  if (!bpg::tree_plan(c.n, c.shape, &plan)) return complain(c, "no plan");
  const std::vector<std::pair<uint32_t, uint32_t>> plan_copy = plan;
  const uint32_t total = c.n + (uint32_t)plan.size();
  Record rec(total);
  // a batch that carries the failing job fails as a whole, as a lock-step batch does
  auto carries_failure = [&](const std::vector<std::unique_ptr<bpg::RecJob>>& jobs) {
    for (auto& j : jobs)
      if ((int)j->node == c.fail_job) return true;
    return false;
  };
  bpg::TreeOps ops;
  ops.cap = CAP;
  ops.pooled = c.pooled;
  ops.last_error = [] { return t_error; };
  ops.leaf = [&](uint32_t i, bpg::RecPool* pool, uint8_t** out, size_t* out_len, bool* posted) {
    InCallback in(rec);
    if ((int)i == c.fail_leaf) return fail_with(BP_ERR_RANGE, "leaf " + std::to_string(i) + " is out of range");
    if (!pool) {  // proved on the spot
      rec.made[i]++;
      *out = box_of(i, out_len);
      return (int)BP_OK;
    }
    for (int level = 0; level < 3; level++) {
      std::vector<std::unique_ptr<bpg::RecJob>> riders;
      pool->take(CAP - HOSTS, &riders);
      rec.batch((int)(HOSTS + riders.size()));
      rec.rider_slots += (int)riders.size();
      if (carries_failure(riders)) return fail_with(BP_ERR_VERIFY, "a rider failed");
      for (auto& j : riders) {
        rec.made[j->node]++;
        size_t len = 0;
        uint8_t* b = box_of(j->node, &len);
        pool->complete(*j, b, len);
      }
      std::this_thread::yield();
    }
    std::unique_ptr<bpg::RecJob> job(new bpg::RecJob());
    job->node = i;
    job->kind = 0;
    pool->post(std::move(job));
    *posted = true;
    return (int)BP_OK;
  };
  auto children_ok = [&](uint32_t nid, const bpg::TreeBuf& l, const bpg::TreeBuf& r, int la, int ra) {
    const auto& pr = plan_copy[nid - c.n];
    if (node_of(l) != pr.first || node_of(r) != pr.second) rec.bad++;  // a child that is not there yet, or another node's
    if (la != (pr.first >= c.n) || ra != (pr.second >= c.n)) rec.bad++;
  };
  ops.agg_prepare = [&](const bpg::TreeBuf& l, int la, const bpg::TreeBuf& r, int ra, bpg::RecJob* job) {
    InCallback in(rec);
    children_ok(job->node, l, r, la, ra);
    job->kind = 1;
    return (int)BP_OK;
  };
  ops.agg = [&](const bpg::TreeBuf& l, int la, const bpg::TreeBuf& r, int ra, uint8_t** out, size_t* out_len) {
    InCallback in(rec);
    // the node is the parent of its left child
    uint32_t nid = ~0u;
    for (uint32_t k = 0; k < plan_copy.size(); k++)
      if (plan_copy[k].first == node_of(l)) nid = c.n + k;
    if (nid == ~0u) { rec.bad++; return fail_with(BP_ERR_DEVICE, "an aggregation of no node"); }
    children_ok(nid, l, r, la, ra);
    rec.made[nid]++;
    *out = box_of(nid, out_len);
    return (int)BP_OK;
  };
  ops.prove_batch = [&](const std::vector<std::unique_ptr<bpg::RecJob>>& jobs, std::vector<bpg::TreeBuf>* out) {
    InCallback in(rec);
    rec.batch((int)jobs.size());
    rec.drained += (int)jobs.size();
    if (carries_failure(jobs)) return fail_with(BP_ERR_VERIFY, "a rider failed");
    for (size_t k = 0; k < jobs.size(); k++) {
      if (k && std::make_pair(jobs[k - 1]->kind == 1 ? 0 : 1, jobs[k - 1]->node) >= std::make_pair(jobs[k]->kind == 1 ? 0 : 1, jobs[k]->node))
        rec.bad++;  // aggregations before roots, each in node order
      rec.made[jobs[k]->node]++;
      bpg::TreeBuf b;
      b.p = box_of(jobs[k]->node, &b.n);
      out->push_back(b);
    }
    return (int)BP_OK;
  };
  bpg::TreeRun run(c.n, std::move(plan), ops, nullptr, nullptr, c.keep_leaves);
  const int rc = run.run(c.threads);
  if (rec.in_callback.load() != 0) return complain(c, "a thread was still in a callback when run() returned");
  if (rec.max_batch.load() > (int)CAP) return complain(c, "a batch exceeds 8");
  if (rec.bad.load()) return complain(c, "an aggregation saw the wrong children, or a batch was out of order");
  if (c.fail_leaf >= 0 || c.fail_job >= 0) {
    const int want = c.fail_leaf >= 0 ? BP_ERR_RANGE : BP_ERR_VERIFY;
    const std::string msg = c.fail_leaf >= 0 ? "leaf " + std::to_string(c.fail_leaf) + " is out of range" : "a rider failed";
    if (rc != want) return complain(c, "the failure's status was lost");
    if (run.error() != msg) return complain(c, "the failure's message was lost");
    for (auto& m : rec.made)
      if (m.load() > 1) return complain(c, "a node was completed twice");
    return true;
  }
  if (rc != BP_OK) return complain(c, run.error().c_str());
  for (uint32_t k = 0; k < total; k++)
    if (rec.made[k].load() != 1) return complain(c, "a node was not completed exactly once");
  if (node_of(run.result(run.root())) != total - 1) return complain(c, "the root's container is not the root's");
  if (c.keep_leaves && c.n > 1)
    for (uint32_t i = 0; i < c.n; i++)
      if (node_of(run.result(i)) != i) return complain(c, "a leaf the caller wanted was freed");
  if (c.pooled && rec.rider_slots.load() + rec.drained.load() != (int)total) return complain(c, "jobs were neither ridden nor drained");
  return true;
}

}  // namespace

int main() {
  const uint32_t sizes[] = {1, 2, 3, 5, 8, 13, 32}, threads[] = {1, 2, 4};
  int cases = 0, failed = 0;
  for (uint32_t n : sizes)
    for (uint32_t t : threads)
      for (uint32_t shape = 0; shape < 2; shape++)
        for (int pooled = 0; pooled < 2; pooled++) {
          Case c{n, t, shape, pooled != 0, (n + t) % 2 == 0};
          cases++;
          failed += !run_case(c);
          // a failing leaf (the last one: everything before it is under way), and a failing job (a root in the middle,
          // and the first aggregation)
          Case fl = c;
          fl.fail_leaf = (int)n - 1;
          cases++;
          failed += !run_case(fl);
          if (pooled) {
            Case fj = c;
            fj.fail_job = (int)(n / 2);
            cases++;
            failed += !run_case(fj);
            if (n > 1) {
              Case fa = c;
              fa.fail_job = (int)n;
              cases++;
              failed += !run_case(fa);
            }
          }
        }
  std::printf("%d cases, %d failed\n", cases, failed);
  return failed ? 1 : 0;
}
