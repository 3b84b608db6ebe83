// caller_table.cpp -- the one path behind the entries that take a caller's table (caller_table.hpp).
#include <cstdlib>
#include <mutex>
#include <string>
#include "caller_table.hpp"

namespace bpg {

int check_public_inputs(const char* who, const char* where, const CallerTable& t) {
  if (!t.pub) return t.reads_public() ? fail(BP_ERR_INVALID_INPUT, "%s: %sthe AIR reads public inputs: pass four words", who, where) : BP_OK;
  for (int j = 0; j < 4; j++)
    if (t.pub[j] >= gl::P) return fail(BP_ERR_INVALID_INPUT, "%s: %snon-canonical public input", who, where);
  return BP_OK;
}
int check_caller_table(const char* who, const char* where, const CallerTable& t) {
  const uint64_t N = (uint64_t)1 << t.cfg.log_n;
  if (!t.trace) return fail(BP_ERR_INVALID_INPUT, "%s: %snull trace", who, where);
  if (t.stride < N)
    return fail(BP_ERR_INVALID_INPUT, "%s: %scolumn stride %llu is shorter than the %llu-row trace", who, where, (unsigned long long)t.stride,
                (unsigned long long)N);
  if (t.cfg.n_const && !t.consts)
    return fail(BP_ERR_INVALID_INPUT, "%s: %sthe AIR reads %u constant columns: pass them", who, where, t.cfg.n_const);
  return check_public_inputs(who, where, t);
}

size_t table_arena_bytes(const StarkCfg& c, bool packed) {
  const uint64_t N = (uint64_t)1 << c.log_n, M = N << c.rate_bits;
  const size_t cols = (size_t)c.n_cols + c.n_const + c.n_cols / 8 + (2u << c.rate_bits) + 64;
  return cols * (2 * N + M) * 8 + (size_t)80 * M * 8 + ((size_t)c.n_cols / 32 + 64) * 8 * N * 8 + (packed ? (size_t)c.n_cols * N * 8 : 0);
}

namespace {
std::mutex g_park_mu;
std::vector<Worker*> g_parked;  // index = device

void drop(Worker* w) {
  w->destroy();
  delete w;
}
void park_worker(Worker* w) {
  {
    std::lock_guard<std::mutex> lk(g_park_mu);
    if (w->device >= 0) {
      if (g_parked.size() <= (size_t)w->device) g_parked.resize(w->device + 1, nullptr);
      if (!g_parked[w->device]) {
        g_parked[w->device] = w;
        return;
      }
    }
  }
  drop(w);
}
}  // namespace

WorkerLease::WorkerLease(int device, size_t bytes) {
  Worker* w = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_park_mu);
    if (device >= 0 && (size_t)device < g_parked.size() && g_parked[device]) {
      w = g_parked[device];
      g_parked[device] = nullptr;
    }
  }
  if (w && w->arena.capacity() >= bytes) {
    if (hipSetDevice(device) != hipSuccess) {
      rc_ = fail(BP_ERR_DEVICE, "hipSetDevice(%d) failed", device);
      park_worker(w);
      return;
    }
    w->arena.release(0);
    w->abort_flag = nullptr;
    w_ = w;
    return;
  }
  if (w) drop(w);
  w = new Worker();
  if ((rc_ = w->init(device, bytes))) drop(w);
  else w_ = w;
}
WorkerLease::~WorkerLease() {
  if (w_) park_worker(w_);
}
void release_parked_workers() {
  std::vector<Worker*> all;
  {
    std::lock_guard<std::mutex> lk(g_park_mu);
    all.swap(g_parked);
  }
  for (Worker* w : all)
    if (w) drop(w);
}

int commit_caller_table(Worker& w, Challenger& ch, const CallerTable& t, Committed* consts, Committed* trace, const uint64_t** d_values) {
  const StarkCfg& c = t.cfg;
  const uint64_t N = (uint64_t)1 << c.log_n;
  if (c.n_const) {
    if (int rc = commit(w, t.consts, c.n_const, c.log_n, c.rate_bits, c.cap_height, false, consts)) return rc;
    ch.observe(consts->cap.data(), consts->cap.size());
  }
  *d_values = t.trace;
  if (t.stride != N) {
    uint64_t* packed = w.arena.alloc_words((size_t)c.n_cols * N);
    if (!packed) return fail(BP_ERR_DEVICE, "arena exhausted");
    BPG_HIP(hipMemcpy2DAsync(packed, N * 8, t.trace, t.stride * 8, N * 8, c.n_cols, hipMemcpyDeviceToDevice, w.stream));
    *d_values = packed;
  }
  if (int rc = commit(w, *d_values, c.n_cols, c.log_n, c.rate_bits, c.cap_height, false, trace)) return rc;
  ch.observe(trace->cap.data(), trace->cap.size());
  return BP_OK;
}

int emit(const std::vector<uint64_t>& words, uint8_t** out, size_t* out_len) {
  *out = static_cast<uint8_t*>(std::malloc(words.size() * 8));
  if (!*out) return fail(BP_ERR_DEVICE, "host allocation failed");
  *out_len = words.size() * 8;
  std::memcpy(*out, words.data(), *out_len);
  return BP_OK;
}
int finish(Worker& w, int rc, uint8_t** out, size_t* out_len) {
  if (rc) {
    const std::string why = bp_last_error();  // (no later call may lose the message)
    (void)hipStreamSynchronize(w.stream);
    return fail(rc, "%s", why.c_str());
  }
  if ((rc = w.wait())) {
    std::free(*out);
    *out = nullptr;
    *out_len = 0;
  }
  return rc;
}

}  // namespace bpg
