// pb_memory.hpp -- who owns what the engine allocates: move-only owners of device memory, pinned host memory, events
// and streams.  An owner releases what it holds when it is destroyed or assigned a fresh value, so "switch it off" is an
// assignment and a batch's destructor names no buffer.  Errors of a release are ignored.  No kernel code here.
#pragma once

#include <atomic>
#include <cstddef>
#include <utility>

#include <hip/hip_runtime_api.h>

// live allocations made through the device and the pinned traits, process-wide (pbDeviceMemoryLive)
struct PbMemoryLive {
  static inline std::atomic<unsigned long long> buffers{0}, bytes{0};
};

struct PbDeviceTraits {
  static constexpr bool counted = true;
  static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
  static hipError_t free(void *p) { return hipFree(p); }
};
struct PbPinnedTraits {
  static constexpr bool counted = true;
  static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes); }
  static hipError_t free(void *p) { return hipHostFree(p); }
};

// `capacity()` elements of T from Traits::alloc(void **, bytes), given back through Traits::free(void *); both return a
// hipError_t.  Traits::counted: the block shows in PbMemoryLive.
template <typename T, typename Traits>
class PbOwned {
 public:
  PbOwned() = default;
  PbOwned(PbOwned &&o) noexcept { swap(o); }
  PbOwned &operator=(PbOwned &&o) noexcept {
    PbOwned(std::move(o)).swap(*this);  // (what was held goes with the temporary)
    return *this;
  }
  ~PbOwned() { reset(); }
  void swap(PbOwned &o) noexcept {
    std::swap(p_, o.p_);
    std::swap(count_, o.count_);
  }

  // frees what is held, then holds `count` fresh elements; on an error the owner is empty
  hipError_t alloc(size_t count) {
    reset();
    void *p = nullptr;
    const hipError_t e = Traits::alloc(&p, sizeof(T) * count);
    if (e != hipSuccess || !p) return e;
    p_ = (T *)p, count_ = count;
    if (Traits::counted) PbMemoryLive::buffers += 1, PbMemoryLive::bytes += sizeof(T) * count;
    return hipSuccess;
  }
  // nothing when `count` elements fit; else alloc(count): the contents are not kept
  hipError_t ensure(size_t count) { return count <= count_ ? hipSuccess : alloc(count); }
  void reset() {
    if (!p_) return;
    (void)Traits::free(p_);
    if (Traits::counted) PbMemoryLive::buffers -= 1, PbMemoryLive::bytes -= sizeof(T) * count_;
    p_ = nullptr, count_ = 0;
  }
  size_t capacity() const { return count_; }
  T *get() const { return p_; }
  operator T *() const { return p_; }  // launches, pointer arithmetic and null tests read as with a raw pointer

 private:
  T *p_ = nullptr;
  size_t count_ = 0;
};

template <typename T>
using PbDevBuf = PbOwned<T, PbDeviceTraits>;
template <typename T>
using PbPinned = PbOwned<T, PbPinnedTraits>;

// A HIP handle (an event, a stream) destroyed with Destroy when set.
template <typename Handle, hipError_t (*Destroy)(Handle)>
class PbHandle {
 public:
  PbHandle() = default;
  PbHandle(PbHandle &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  PbHandle &operator=(PbHandle &&o) noexcept {
    PbHandle old(std::move(o));
    std::swap(h_, old.h_);
    return *this;
  }
  ~PbHandle() { reset(); }
  void reset() {
    if (h_) (void)Destroy(h_);
    h_ = nullptr;
  }
  operator Handle() const { return h_; }

 protected:
  Handle h_ = nullptr;
};

struct PbEvent : PbHandle<hipEvent_t, hipEventDestroy> {
  hipError_t create() {
    reset();
    return hipEventCreate(&h_);
  }
};
// The device time of the last span of launches that start() and stop() bracketed on a stream.  Neither waits; ms()
// waits for the span's end.  The events are made by the first start.
class PbSpanClock {
 public:
  hipError_t start(hipStream_t stream) {
    hipError_t e = hipSuccess;
    if (!ev0_) e = ev0_.create();
    if (e == hipSuccess && !ev1_) e = ev1_.create();
    return e != hipSuccess ? e : hipEventRecord(ev0_, stream);
  }
  hipError_t stop(hipStream_t stream) {
    const hipError_t e = hipEventRecord(ev1_, stream);
    if (e == hipSuccess) timed_ = true;
    return e;
  }
  bool timed() const { return timed_; }  // a span was recorded: ms() will touch the device
  // 0 before any span; else the last span's device time, once its end has passed
  hipError_t ms(float *out) const {
    *out = 0.0f;
    if (!timed_) return hipSuccess;
    const hipError_t e = hipEventSynchronize(ev1_);
    return e != hipSuccess ? e : hipEventElapsedTime(out, ev0_, ev1_);
  }

 private:
  PbEvent ev0_, ev1_;
  bool timed_ = false;
};
struct PbStream : PbHandle<hipStream_t, hipStreamDestroy> {
  hipError_t create(unsigned flags) {
    reset();
    return hipStreamCreateWithFlags(&h_, flags);
  }
};
