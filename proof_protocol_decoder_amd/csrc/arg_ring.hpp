// arg_ring.hpp -- where the argument blocks of the batched kernels live between the launch and the kernel's end.
//
// A kernel that runs `batch` proofs in lock-step reads one argument block per proof (stark_kernels.hpp: QuotArgs,
// FriLayerArgs, ...).  The blocks used to travel in the kernel-argument segment, which holds 4 KiB: eight proofs at
// most.  They now lie in memory the host writes and the device reads (host-pinned, device-mapped, as a worker's
// mailbox is), one piece per stream, and the kernel is handed a pointer.  This is the bookkeeping of that piece:
//
//  * put: copies n blocks behind the blocks already there and answers with the DEVICE address of the copy.  Blocks are
//    never moved or overwritten while they are live, i.e. until
//  * rewind: the owner has waited for its stream -- every launch that read a block has completed -- and the piece is
//    empty again (Worker::wait, prover.cpp).
//  * A put that does not fit asks for that wait first (the `wait` the caller hands in: wait for the stream, nothing
//    else) and rewinds; blocks larger than the whole piece are refused.
//
// Every block starts on an ALIGN boundary of both views (the two views of the memory have the same alignment: both are
// page-aligned).  One thread uses a ring at a time: the one that holds the worker, or the lane, it belongs to.
// Plain C++, no HIP: it is handed its memory; tools/arg_ring_check.cpp runs it under the address sanitizer.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace bpg {

// No per-proof block is larger than this (stark_kernels.hip asserts it of every block type), and the two blocks that
// hold a whole batch -- the query launches', with their index arrays -- stay within ARG_WHOLE_MAX.
constexpr size_t ARG_BLOCK_MAX = 384;
constexpr size_t ARG_WHOLE_MAX = 12 << 10;

class ArgRing {
 public:
  static constexpr size_t ALIGN = 64;
  enum Status { OK = 0, WAIT_FAILED = 1, TOO_LARGE = 2, NO_MEMORY = 3 };

  // host / dev: the two views of `bytes` bytes of memory the caller owns (dev == host where there is one view), both
  // starting on an ALIGN boundary -- memory that does not is not taken (capacity 0: every put answers NO_MEMORY)
  void adopt(void* host, void* dev, size_t bytes) {
    host_ = static_cast<char*>(host);
    dev_ = static_cast<char*>(dev);
    const bool aligned = reinterpret_cast<uintptr_t>(host) % ALIGN == 0 && reinterpret_cast<uintptr_t>(dev) % ALIGN == 0;
    cap_ = host && dev && aligned ? bytes & ~(ALIGN - 1) : 0;
    off_ = high_ = 0;
    n_waits_ = 0;
  }
  void forget() { adopt(nullptr, nullptr, 0); }
  size_t capacity() const { return cap_; }
  size_t used() const { return off_; }
  size_t high_water() const { return high_; }
  uint64_t waits() const { return n_waits_; }  // puts that found the ring full
  static constexpr size_t padded(size_t bytes) { return (bytes + ALIGN - 1) & ~(ALIGN - 1); }
  bool fits(size_t bytes) const { return bytes <= cap_ && padded(bytes) <= cap_ - off_; }

  // every earlier launch of the stream has completed: nothing is live
  void rewind() { off_ = 0; }

  // `bytes` bytes of blocks -> *dev_out, their device address.  wait(): 0 once the stream has drained.
  template <class Wait>
  Status put(const void* blocks, size_t bytes, const void** dev_out, Wait&& wait) {
    *dev_out = nullptr;
    if (!cap_) return NO_MEMORY;
    if (bytes > cap_) return TOO_LARGE;
    if (!fits(bytes)) {
      n_waits_++;
      if (wait() != 0) return WAIT_FAILED;
      rewind();
    }
    std::memcpy(host_ + off_, blocks, bytes);
    *dev_out = dev_ + off_;
    off_ += padded(bytes);
    if (off_ > high_) high_ = off_;
    return OK;
  }

 private:
  char *host_ = nullptr, *dev_ = nullptr;
  size_t cap_ = 0, off_ = 0, high_ = 0;
  uint64_t n_waits_ = 0;
};

}  // namespace bpg
