// arg_ring_check.cpp -- the argument ring's bookkeeping (csrc/arg_ring.hpp) on the CPU, with a fake stream.
//
// No device, no library.  The ring is handed two views of one heap buffer that differ by a fixed distance (the "device"
// view is never dereferenced as such: a block's device address minus that distance is where the host wrote it).  A fake
// stream counts launches that are queued and not yet complete; a block is LIVE from its put until the wait that follows
// it, and every live block is checked, byte for byte, after every later put: nothing overwrote it.
//
//  * alignment: every device address is a multiple of ArgRing::ALIGN, whatever the sizes put before it;
//  * puts of 1, 8, 9 and 24 blocks of the largest per-proof block (ARG_BLOCK_MAX) and of one whole-batch block
//    (ARG_WHOLE_MAX), alone and mixed, into rings of several sizes;
//  * the full case: a put that does not fit asks for exactly one wait, then starts at the front, and it never lands
//    on a block that is live -- the wait is what ended their lives;
//  * rewind after a wait: the next put is at the front again and the whole capacity is free;
//  * a block larger than the ring is refused (TOO_LARGE), without a wait and without touching what is live; a ring with
//    no memory refuses everything; a wait that fails fails the put and writes nothing.
// Built by tests/test_arg_ring_host.py, plain and with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "../proof_protocol_decoder_amd/csrc/arg_ring.hpp"

namespace {

using bpg::ArgRing;

int n_cases = 0, n_failed = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    n_cases++;                                                            \
    if (!(cond)) {                                                        \
      n_failed++;                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
    }                                                                     \
  } while (0)

constexpr ptrdiff_t DEV_SHIFT = (ptrdiff_t)1 << 40;  // a multiple of every alignment: the views agree in theirs

struct Live {
  size_t off, bytes;
  uint8_t fill;
};

struct AlignedMem {  // page-aligned, as pinned memory is
  char* p = nullptr;
  size_t n = 0;
  explicit AlignedMem(size_t bytes) : n(bytes) {
    void* q = nullptr;
    if (posix_memalign(&q, 4096, bytes ? bytes : 1) != 0) std::abort();
    p = static_cast<char*>(q);
    std::memset(p, 0, bytes);
  }
  AlignedMem(const AlignedMem&) = delete;
  AlignedMem& operator=(const AlignedMem&) = delete;
  ~AlignedMem() { std::free(p); }
  char* data() const { return p; }
  size_t size() const { return n; }
  char operator[](size_t k) const { return p[k]; }
};

struct Harness {
  AlignedMem mem;
  ArgRing ring;
  std::vector<Live> live;
  int waits = 0;
  bool wait_fails = false;
  uint8_t next_fill = 1;

  explicit Harness(size_t bytes) : mem(bytes) {
    ring.adopt(mem.data(), reinterpret_cast<char*>(reinterpret_cast<uintptr_t>(mem.data()) + DEV_SHIFT), bytes);
  }
  int wait() {
    waits++;
    if (wait_fails) return 1;
    live.clear();  // every queued launch has completed: no block is read any more
    return 0;
  }
  bool live_intact() const {
    for (const Live& l : live)
      for (size_t k = 0; k < l.bytes; k++)
        if ((uint8_t)mem[l.off + k] != l.fill) return false;
    return true;
  }
  // one launch's blocks; answers the ring's status and checks everything that must hold after any put
  ArgRing::Status put(size_t bytes) {
    std::vector<char> blocks(bytes, (char)next_fill);
    const void* dev = nullptr;
    const size_t used_before = ring.used();
    const int waits_before = waits;
    const ArgRing::Status st = ring.put(blocks.data(), bytes, &dev, [this] { return wait(); });
    if (st == ArgRing::OK) {
      const char* host = reinterpret_cast<const char*>(reinterpret_cast<uintptr_t>(dev) - DEV_SHIFT);
      const size_t off = (size_t)(host - mem.data());
      CHECK(dev != nullptr && host >= mem.data() && off + bytes <= mem.size());
      CHECK(reinterpret_cast<uintptr_t>(dev) % ArgRing::ALIGN == 0 && off % ArgRing::ALIGN == 0);
      CHECK(waits - waits_before <= 1);
      if (waits == waits_before) CHECK(off == used_before);  // behind what was there
      else CHECK(off == 0);                                   // the wait emptied the ring
      for (const Live& l : live) CHECK(off >= l.off + l.bytes || off + bytes <= l.off);  // no overlap with a live block
      live.push_back(Live{off, bytes, next_fill});
      next_fill = next_fill == 255 ? 1 : next_fill + 1;
    } else {
      CHECK(dev == nullptr);
      CHECK(ring.used() == used_before || (st == ArgRing::WAIT_FAILED && waits == waits_before + 1));
    }
    CHECK(live_intact());
    CHECK(ring.used() <= ring.capacity() && ring.high_water() <= ring.capacity());
    return st;
  }
  // Worker::wait: the stream has drained, the ring is empty
  void owner_wait() {
    live.clear();
    ring.rewind();
  }
};

void sizes_and_alignment() {
  const size_t block = bpg::ARG_BLOCK_MAX;
  for (size_t cap : {(size_t)16 << 10, (size_t)64 << 10, (size_t)1 << 20}) {
    Harness h(cap);
    for (uint32_t n : {1u, 8u, 9u, 24u}) CHECK(h.put(n * block) == ArgRing::OK);
    CHECK(h.put(bpg::ARG_WHOLE_MAX) == ArgRing::OK);
    CHECK(h.put(1) == ArgRing::OK);
    CHECK(h.put(63) == ArgRing::OK);
    CHECK(h.put(65) == ArgRing::OK);
    CHECK(h.put(24 * block) == ArgRing::OK);
    h.owner_wait();
    CHECK(h.ring.used() == 0);
    CHECK(h.put(24 * block) == ArgRing::OK && h.live.back().off == 0);  // rewind after a wait: at the front again
  }
}

void full_case() {
  const size_t block = bpg::ARG_BLOCK_MAX;
  Harness h(32 << 10);  // three launches of 24 blocks fit, the fourth does not
  for (int k = 0; k < 3; k++) CHECK(h.put(24 * block) == ArgRing::OK);
  CHECK(h.waits == 0 && h.live.size() == 3);
  CHECK(!h.ring.fits(24 * block));
  CHECK(h.put(24 * block) == ArgRing::OK);
  CHECK(h.waits == 1 && h.live.size() == 1 && h.live[0].off == 0 && h.ring.waits() == 1);
  // a small put still fits behind it without a wait
  CHECK(h.put(block) == ArgRing::OK && h.waits == 1);
  // exactly full, then one byte more
  Harness e(4096);
  CHECK(e.put(4096 - 64) == ArgRing::OK && e.put(64) == ArgRing::OK && e.waits == 0 && e.ring.used() == 4096);
  CHECK(e.put(1) == ArgRing::OK && e.waits == 1 && e.ring.used() == 64);
  // a wait that fails: the put fails, nothing is written, the live blocks stay as they are
  Harness f(4096);
  CHECK(f.put(4000) == ArgRing::OK);
  f.wait_fails = true;
  CHECK(f.put(200) == ArgRing::WAIT_FAILED && f.live.size() == 1 && f.live_intact());
  f.wait_fails = false;
  CHECK(f.put(200) == ArgRing::OK && f.waits == 2);
}

void refusals() {
  Harness h(8192);
  CHECK(h.put(100) == ArgRing::OK);
  CHECK(h.put(8193) == ArgRing::TOO_LARGE && h.waits == 0 && h.live.size() == 1);
  CHECK(h.put(24 * bpg::ARG_BLOCK_MAX) == ArgRing::TOO_LARGE && h.waits == 0);  // 9216 bytes
  CHECK(h.put(8192) == ArgRing::OK && h.waits == 1);                            // the whole ring: after a wait
  ArgRing none;
  const void* dev = &none;
  char b = 0;
  CHECK(none.put(&b, 1, &dev, [] { return 0; }) == ArgRing::NO_MEMORY && dev == nullptr);
  // a capacity that is no multiple of ALIGN counts down to one
  AlignedMem mem(1000);
  ArgRing odd;
  odd.adopt(mem.data(), mem.data(), mem.size());
  CHECK(odd.capacity() == 960);
  // ... and memory that does not start on an ALIGN boundary is not taken at all
  odd.adopt(mem.data() + 8, mem.data() + 8, 512);
  CHECK(odd.capacity() == 0 && odd.put(&b, 1, &dev, [] { return 0; }) == ArgRing::NO_MEMORY);
}

void random_traffic() {
  std::mt19937 g(12345);
  for (size_t cap : {(size_t)4096, (size_t)20000, (size_t)1 << 18}) {
    Harness h(cap);
    for (int k = 0; k < 4000; k++) {
      const uint32_t kind = g() % 16;
      if (kind == 0) { h.owner_wait(); continue; }
      const size_t bytes = kind == 1 ? bpg::ARG_WHOLE_MAX : kind == 2 ? cap + 1 + g() % 100 : (1 + g() % 24) * (size_t)(8 + g() % (bpg::ARG_BLOCK_MAX - 7));
      const ArgRing::Status st = h.put(bytes);
      CHECK(st == (bytes > h.ring.capacity() ? ArgRing::TOO_LARGE : ArgRing::OK));
    }
    CHECK(h.ring.high_water() <= cap);
  }
}

}  // namespace

int main() {
  sizes_and_alignment();
  full_case();
  refusals();
  random_traffic();
  std::printf("%d cases, %d failed\n", n_cases, n_failed);
  return n_failed ? 1 : 0;
}
