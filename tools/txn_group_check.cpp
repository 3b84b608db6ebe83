// txn_group_check.cpp -- groups of transactions (Tune::txn_group) on the CPU: the shard scheduler's group rule
// (csrc/rec_pool.hpp) and the group lease's worker table (csrc/worker_table.hpp), with fake provers.
//
// No device, no library.  The lease is the real bookkeeping -- bpg::WorkerTable under a mutex and a condition variable,
// used exactly as proofgen.cpp's WorkerLease / GroupLease use it: wait while NO worker is idle, take, work, give back --
// behind a fake worker table whose "arena" is the worker's index.  A fake container is the id of its node.
//
//  Scheduler: n = 1..40 leaves x 1..8 threads x group sizes 1..3 x worker counts, pooled and not; leases that grant
//  fewer than they are asked for (few workers, single leases of the drained batches in between, and a lease that is
//  made to grant one); a failing member; an abort in mid-run.  Checked from the data the scheduler moved:
//   * every node is completed exactly once, the root's container is the root's;
//   * a group is offered at most `group` leaves, ascending; the leaves it does not take are started later, by someone
//     (handed back), and with one thread the leaves start in index order;
//   * no worker is granted twice at a time, the workers of a group are neighbours in one slab (the span equals the
//     slices granted), and never more transactions are under way than there are workers;
//   * a failure's or an abort's status and message are the run's, with every thread joined.
//  Lease: threads that take runs of 1..3 and threads that take single workers, side by side, on tables of 1..9 workers
//  in one, two and three slabs: no double grant, adjacency, all-or-the-longest-run, and it ends (no deadlock).
// Built by tests/test_txn_group_host.py with -fsanitize=thread and, a second time, -fsanitize=address,undefined.
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <mutex>
#include "../proof_protocol_decoder_amd/csrc/rec_pool.hpp"
#include "../proof_protocol_decoder_amd/csrc/worker_table.hpp"

namespace {

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

// the state's side of a lease, as proofgen.cpp has it
struct FakeState {
  std::mutex mu;
  std::condition_variable cv;
  bpg::WorkerTable table;
  std::vector<std::atomic<int>> held;  // per worker: leases that hold it right now (must never pass 1)
  std::atomic<int> bad{0}, in_flight{0}, max_in_flight{0};
  explicit FakeState(const std::vector<uint32_t>& slab_of) : held(slab_of.size()) {
    table.reset(slab_of);
    for (auto& h : held) h.store(0);
  }
  void hold(uint32_t first, uint32_t n) {
    for (uint32_t k = 0; k < n; k++) {
      if (held[first + k].fetch_add(1) != 0) bad++;                  // a double grant
      if (k && !table.adjacent(first + k - 1, first + k)) bad++;      // the span is not the slices granted
    }
    const int now = in_flight.fetch_add((int)n) + (int)n;
    int cur = max_in_flight.load();
    while (now > cur && !max_in_flight.compare_exchange_weak(cur, now)) {
    }
    if (now > (int)held.size()) bad++;
  }
  uint32_t lease_run(uint32_t want, uint32_t* first) {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return table.any_idle(); });
    // all or the longest run: what take_run must give, counted before it changes the table
    uint32_t longest = 0;
    for (uint32_t i = 0, len = 0; i < table.size(); i++) {
      len = table.idle(i) ? ((i && table.idle(i - 1) && table.adjacent(i - 1, i)) ? len + 1 : 1) : 0;
      longest = std::max(longest, len);
    }
    const uint32_t n = table.take_run(want, first);
    if (n != std::min(want, longest)) bad++;
    hold(*first, n);
    return n;
  }
  uint32_t lease_one() {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return table.any_idle(); });
    const int i = table.take_one();
    if (i < 0) { bad++; return 0; }
    hold((uint32_t)i, 1);
    return (uint32_t)i;
  }
  void give(uint32_t first, uint32_t n) {
    in_flight.fetch_sub((int)n);
    for (uint32_t k = 0; k < n; k++) held[first + k].fetch_sub(1);
    std::lock_guard<std::mutex> lk(mu);
    for (uint32_t k = 0; k < n; k++) table.give(first + k);
    cv.notify_all();
  }
};

std::vector<uint32_t> slabs_of(uint32_t n_workers, uint32_t n_slabs) {
  std::vector<uint32_t> s(n_workers);
  for (uint32_t i = 0; i < n_workers; i++) s[i] = i * n_slabs / n_workers;
  return s;
}

struct Case {
  uint32_t n, threads, group, workers, slabs;
  bool pooled;
  int fail_leaf = -1;    // the group that holds this leaf returns BP_ERR_RANGE
  int abort_after = -1;  // the abort flag is raised when this many leaves have been started
  bool stingy = false;   // every lease grants one worker
};
bool complain(const Case& c, const char* what) {
  std::printf("FAILED n=%u threads=%u group=%u workers=%u slabs=%u pooled=%d fail_leaf=%d abort_after=%d stingy=%d: %s\n", c.n, c.threads,
              c.group, c.workers, c.slabs, (int)c.pooled, c.fail_leaf, c.abort_after, (int)c.stingy, what);
  return false;
}

bool run_case(const Case& c) {
  std::vector<std::pair<uint32_t, uint32_t>> plan;
  if (!bpg::tree_plan(c.n, 0, &plan)) return complain(c, "no plan");
  const uint32_t total = c.n + (uint32_t)plan.size();
  FakeState st(slabs_of(c.workers, c.slabs));
  std::vector<std::atomic<int>> made(total), started(c.n);
  for (auto& m : made) m.store(0);
  for (auto& m : started) m.store(0);
  std::atomic<int> bad{0}, n_started{0}, in_callback{0};
  std::mutex order_mu;
  std::vector<uint32_t> start_order;
  volatile uint8_t abort_flag = 0;
  struct In {
    std::atomic<int>& c;
    explicit In(std::atomic<int>& x) : c(x) { c++; }
    ~In() { c--; }
  };
  bpg::TreeOps ops;
  ops.cap = 8;
  ops.pooled = c.pooled;
  ops.group = c.group;
  ops.lanes = c.workers;
  ops.last_error = [] { return t_error; };
  const auto group_fn = [&](const uint32_t* ids, uint32_t n, bpg::RecPool* pool, const std::function<void(uint32_t)>& granted, bpg::TreeBuf* outs) {
    In in(in_callback);
    if (n < 1 || n > c.group) bad++;
    for (uint32_t k = 1; k < n; k++)
      if (ids[k] <= ids[k - 1]) bad++;
    uint32_t first = 0;
    const uint32_t g = st.lease_run(c.stingy ? 1 : n, &first);
    struct Give {
      FakeState& s;
      uint32_t first, n;
      ~Give() { s.give(first, n); }
    } give{st, first, g};
    granted(g);
    for (uint32_t k = 0; k < g; k++) {
      started[ids[k]]++;
      {
        std::lock_guard<std::mutex> lk(order_mu);
        start_order.push_back(ids[k]);
      }
      if (c.abort_after >= 0 && ++n_started >= c.abort_after) __atomic_store_n(&abort_flag, (uint8_t)1, __ATOMIC_RELAXED);
    }
    for (uint32_t k = 0; k < g; k++)
      if ((int)ids[k] == c.fail_leaf) return fail_with(BP_ERR_RANGE, "leaf " + std::to_string(ids[k]) + " is out of range");
    std::this_thread::yield();
    for (uint32_t k = 0; k < g; k++) {
      if (pool) {
        std::unique_ptr<bpg::RecJob> job(new bpg::RecJob());
        job->node = ids[k];
        job->kind = 0;
        pool->post(std::move(job));
      } else {
        made[ids[k]]++;
        outs[k].p = box_of(ids[k], &outs[k].n);
      }
    }
    return (int)BP_OK;
  };
  ops.leaf_group = group_fn;
  ops.leaf = [&](uint32_t i, bpg::RecPool* pool, uint8_t** out, size_t* out_len, bool* posted) {  // group == 1: one leaf per thread as ever
    if (c.group != 1) bad++;
    bpg::TreeBuf o;
    const int rc = group_fn(&i, 1, pool, [](uint32_t) {}, &o);
    *posted = pool != nullptr;
    *out = o.p;
    *out_len = o.n;
    return rc;
  };
  ops.agg_prepare = [&](const bpg::TreeBuf& l, int, const bpg::TreeBuf& r, int, bpg::RecJob* job) {
    In in(in_callback);
    if (node_of(l) != plan[job->node - c.n].first || node_of(r) != plan[job->node - c.n].second) bad++;
    job->kind = 1;
    return (int)BP_OK;
  };
  ops.agg = [&](const bpg::TreeBuf& l, int, const bpg::TreeBuf&, int, uint8_t** out, size_t* out_len) {
    In in(in_callback);
    uint32_t nid = ~0u;
    for (uint32_t k = 0; k < plan.size(); k++)
      if (plan[k].first == node_of(l)) nid = c.n + k;
    if (nid == ~0u) { bad++; return fail_with(BP_ERR_DEVICE, "an aggregation of no node"); }
    made[nid]++;
    *out = box_of(nid, out_len);
    return (int)BP_OK;
  };
  ops.prove_batch = [&](const std::vector<std::unique_ptr<bpg::RecJob>>& jobs, std::vector<bpg::TreeBuf>* out) {
    In in(in_callback);
    const uint32_t w = st.lease_one();  // a single lease beside the groups, as rec_prove_jobs takes one
    for (auto& j : jobs) {
      made[j->node]++;
      bpg::TreeBuf b;
      b.p = box_of(j->node, &b.n);
      out->push_back(b);
    }
    st.give(w, 1);
    return (int)BP_OK;
  };
  const std::vector<std::pair<uint32_t, uint32_t>> plan_arg = plan;
  bpg::TreeRun run(c.n, plan_arg, ops, c.abort_after >= 0 ? &abort_flag : nullptr, nullptr, false);
  const int rc = run.run(c.threads);
  if (in_callback.load()) return complain(c, "a thread was still in a callback when run() returned");
  if (bad.load() || st.bad.load()) return complain(c, "a group was malformed, or a worker was granted twice, or a span was not adjacent");
  if (st.in_flight.load()) return complain(c, "a lease was not given back");
  for (auto& m : made)
    if (m.load() > 1) return complain(c, "a node was completed twice");
  for (auto& m : started)
    if (m.load() > 1) return complain(c, "a leaf was started twice");
  if (c.fail_leaf >= 0) {
    if (rc != BP_ERR_RANGE || run.error() != "leaf " + std::to_string(c.fail_leaf) + " is out of range") return complain(c, "the failure's status or message was lost");
    return true;
  }
  if (c.abort_after >= 0 && rc == BP_ERR_ABORTED) return run.error().rfind("aborted before", 0) == 0 ? true : complain(c, "the abort's message was lost");
  if (c.abort_after >= 0 && (uint32_t)c.abort_after + c.threads * c.group < c.n) return complain(c, "the abort was not seen");
  if (rc != BP_OK) return complain(c, run.error().c_str());
  for (uint32_t k = 0; k < total; k++)
    if (made[k].load() != 1) return complain(c, "a node was not completed exactly once");
  for (uint32_t i = 0; i < c.n; i++)
    if (started[i].load() != 1) return complain(c, "a leaf that was handed back was never started");
  if (node_of(run.result(run.root())) != total - 1) return complain(c, "the root's container is not the root's");
  if (c.threads == 1)
    for (uint32_t i = 0; i < c.n; i++)
      if (start_order[i] != i) return complain(c, "one thread did not start the leaves in index order (a hand-back out of order)");
  return true;
}

// the lease alone: group leases and single leases side by side
bool lease_case(uint32_t workers, uint32_t slabs, uint32_t threads) {
  FakeState st(slabs_of(workers, slabs));
  std::vector<std::thread> pool;
  std::atomic<int> grants{0};
  for (uint32_t t = 0; t < threads; t++)
    pool.emplace_back([&, t] {
      for (uint32_t it = 0; it < 400; it++) {
        if (t % 3 == 2) {
          const uint32_t w = st.lease_one();
          std::this_thread::yield();
          st.give(w, 1);
        } else {
          uint32_t first = 0;
          const uint32_t n = st.lease_run(1 + (it + t) % 3, &first);
          if (n < 1) st.bad++;
          if (it % 7 == 0) std::this_thread::yield();
          st.give(first, n);
        }
        grants++;
      }
    });
  for (auto& t : pool) t.join();
  if (st.bad.load() || st.in_flight.load() || grants.load() != (int)(threads * 400) || st.table.n_idle() != workers) {
    std::printf("FAILED lease workers=%u slabs=%u threads=%u\n", workers, slabs, threads);
    return false;
  }
  return true;
}

}  // namespace

int main() {
  int cases = 0, failed = 0;
  for (uint32_t n = 1; n <= 40; n++)
    for (uint32_t threads = 1; threads <= 8; threads++) {
      const uint32_t group = 1 + (n + threads) % 3, workers = 1 + (n * 7 + threads * 3) % 8, slabs = 1 + (n + 2 * threads) % std::min<uint32_t>(3, workers);
      for (int pooled = 0; pooled < 2; pooled++) {
        Case c{n, threads, group, workers, slabs, pooled != 0};
        cases++;
        failed += !run_case(c);
      }
      Case g3{n, threads, 3, std::max<uint32_t>(workers, 3), 1, (n & 1) != 0};  // group sizes 1..3 at every n
      for (uint32_t g = 1; g <= 3; g++) {
        g3.group = g;
        cases++;
        failed += !run_case(g3);
      }
      Case st = g3;  // leases that grant fewer than asked: everything but the first leaf is handed back
      st.stingy = true;
      cases++;
      failed += !run_case(st);
      Case fl = g3;  // a failing member (the middle leaf)
      fl.fail_leaf = (int)(n / 2);
      cases++;
      failed += !run_case(fl);
      Case ab = g3;  // an abort in mid-run
      ab.abort_after = (int)(n / 3);
      cases++;
      failed += !run_case(ab);
    }
  for (uint32_t workers = 1; workers <= 9; workers++)
    for (uint32_t slabs = 1; slabs <= std::min<uint32_t>(3, workers); slabs++)
      for (uint32_t threads : {2u, 5u, 8u}) {
        cases++;
        failed += !lease_case(workers, slabs, threads);
      }
  std::printf("%d cases, %d failed\n", cases, failed);
  return failed ? 1 : 0;
}
