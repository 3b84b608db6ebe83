// worker_table.hpp -- which provers of a state are idle, and which of them are neighbours in device memory.
//
// The arenas of a state's workers are slices of a few large device allocations (slabs, proofgen.cpp): slices i and i + 1
// of one slab lie one behind the other, so a prover that leases a RUN of adjacent idle workers owns one contiguous piece
// of memory -- room for several transactions proved in lock-step (Tune::txn_group).  This is the bookkeeping of that:
//
//  * take_one: a single worker, as a ProverLease of one (every call but a group of transactions) and SideLane take one.  An idle worker with no idle
//    neighbour goes first (it is of no use to a group), else the one released last.
//  * take_run: up to `want` adjacent idle workers, all or nothing of ONE run: the shortest run that holds `want`, else
//    the longest run there is (>= 1 while any worker is idle).  It never waits for adjacency.
//  * give: back to idle.
//
// Every call is made under the owner's mutex (bp_state::mu); a caller blocks, on the owner's condition variable, only
// while NO worker is idle, and never while it holds one -- so no thread holds some workers while waiting for others.
// Plain C++, no HIP: tools/txn_group_check.cpp runs it under the thread and address sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace bpg {

class WorkerTable {
 public:
  // slab_of[i]: the allocation worker i's slice lies in; workers i and i + 1 are adjacent iff slab_of agrees
  void reset(std::vector<uint32_t> slab_of) {
    slab_of_ = std::move(slab_of);
    idle_.assign(slab_of_.size(), 1);
    order_.clear();
    for (uint32_t i = 0; i < slab_of_.size(); i++) order_.push_back(i);
  }
  size_t size() const { return slab_of_.size(); }
  bool any_idle() const { return !order_.empty(); }
  size_t n_idle() const { return order_.size(); }
  bool idle(uint32_t i) const { return i < idle_.size() && idle_[i]; }
  bool adjacent(uint32_t i, uint32_t j) const { return j == i + 1 && j < slab_of_.size() && slab_of_[i] == slab_of_[j]; }

  int take_one() {
    if (order_.empty()) return -1;
    size_t pick = order_.size() - 1;
    for (size_t k = order_.size(); k-- > 0;) {
      const uint32_t i = order_[k];
      const bool left = i > 0 && idle_[i - 1] && adjacent(i - 1, i), right = i + 1 < idle_.size() && idle_[i + 1] && adjacent(i, i + 1);
      if (!left && !right) { pick = k; break; }
    }
    const uint32_t i = order_[pick];
    order_.erase(order_.begin() + (std::ptrdiff_t)pick);
    idle_[i] = 0;
    return (int)i;
  }
  // returns the number of workers taken (0 only when none is idle); they are *first .. *first + n - 1
  uint32_t take_run(uint32_t want, uint32_t* first) {
    if (want < 1) want = 1;
    uint32_t best = 0, best_len = 0;
    for (uint32_t i = 0; i < idle_.size();) {
      if (!idle_[i]) { i++; continue; }
      uint32_t j = i + 1;
      while (j < idle_.size() && idle_[j] && adjacent(j - 1, j)) j++;
      const uint32_t len = j - i;
      const bool fits = len >= want, best_fits = best_len >= want;
      if (!best_len || (fits && (!best_fits || len < best_len)) || (!fits && !best_fits && len > best_len)) { best = i; best_len = len; }
      i = j;
    }
    if (!best_len) return 0;
    const uint32_t n = std::min(want, best_len);
    for (uint32_t i = best; i < best + n; i++) {
      idle_[i] = 0;
      order_.erase(std::find(order_.begin(), order_.end(), i));
    }
    *first = best;
    return n;
  }
  void give(uint32_t i) {
    if (i >= idle_.size() || idle_[i]) return;
    idle_[i] = 1;
    order_.push_back(i);
  }

 private:
  std::vector<uint32_t> slab_of_;
  std::vector<char> idle_;
  std::vector<uint32_t> order_;  // the idle workers, the one released last at the back
};

}  // namespace bpg
