// gx_lds_book.hpp -- which (kernel, device) pairs already had their dynamic-LDS limit raised, and to how much.
// Plain C++ on purpose (no HIP include, the setter is passed in): tests/cpp/cudf_host_tests.cpp drives it on the CPU.
// gx_common.hpp's gx::launch_lds is the one user in the library.
#pragma once

#include <atomic>
#include <mutex>
#include <stddef.h>
#include <stdint.h>

namespace gx {

constexpr int LDS_BOOK_DEVICES = 16;    // device ids the book remembers; a higher id is set on every launch
constexpr int LDS_BOOK_SLOTS   = 2048;  // kernels (power of two; the library has a few hundred dynamic-LDS instantiations)

class LdsBook {
 public:
  // Makes sure `set(kernel, bytes)` has succeeded on `device` with at least `bytes`; returns 0 or the setter's error.
  // The record keeps the largest value set, so the setter runs only when a request exceeds every earlier one.  Steady state is one
  // probe of the table and one acquire load.  Raising is serialised by a mutex: the record is published after the setter returned,
  // so no thread sees "set" before it is, and a smaller request can never overwrite a larger one.  A failed set leaves the record
  // as it was (the next request tries again).
  template <typename Setter>
  int ensure(const void* kernel, int device, int bytes, Setter&& set)
  {
    std::atomic<int>* rec = record(kernel, device);
    if (rec && rec->load(std::memory_order_acquire) >= bytes) return 0;
    std::lock_guard<std::mutex> lock(raise_);
    if (rec && rec->load(std::memory_order_relaxed) >= bytes) return 0;
    const int rc = set(kernel, bytes);
    if (rc != 0) return rc;
    if (rec) rec->store(bytes, std::memory_order_release);
    return 0;
  }

 private:
  struct Slot {
    std::atomic<const void*> kernel{nullptr};
    std::atomic<int> bytes[LDS_BOOK_DEVICES] = {};
  };
  // open addressing, insert-only and lock-free; nullptr when the device id or the table is out of room (then: always set)
  std::atomic<int>* record(const void* kernel, int device)
  {
    if (device < 0 || device >= LDS_BOOK_DEVICES) return nullptr;
    size_t i = (size_t)(((uintptr_t)kernel >> 4) * 0x9E3779B97F4A7C15ull >> 32) & (LDS_BOOK_SLOTS - 1);
    for (int probe = 0; probe < LDS_BOOK_SLOTS; ++probe, i = (i + 1) & (LDS_BOOK_SLOTS - 1)) {
      const void* k = slots_[i].kernel.load(std::memory_order_acquire);
      if (k == nullptr && slots_[i].kernel.compare_exchange_strong(k, kernel, std::memory_order_acq_rel)) k = kernel;
      if (k == kernel) return &slots_[i].bytes[device];
    }
    return nullptr;
  }
  Slot slots_[LDS_BOOK_SLOTS];
  std::mutex raise_;
};

}  // namespace gx
