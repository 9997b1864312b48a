// The one owner of device memory: a typed block that frees itself (DESIGN.md "Device memory ownership").
#pragma once
#include <atomic>
#include <type_traits>

#include "common.h"

namespace atdn {

// bytes currently held by DeviceArray objects, process-wide (atdn_device_bytes_live)
inline std::atomic<long long> device_bytes_live{0};

template <class T>
class DeviceArray {
 public:
  T* p = nullptr;
  long n = 0;

  DeviceArray() = default;
  DeviceArray(const DeviceArray&) = delete;
  DeviceArray& operator=(const DeviceArray&) = delete;
  DeviceArray(DeviceArray&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  DeviceArray& operator=(DeviceArray&& o) noexcept {
    if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
    return *this;
  }
  ~DeviceArray() { release(); }

  // Frees what the buffer holds, then allocates `count` elements. A failure throws and leaves the buffer empty.
  // (alloc and release are cold: kept out of line, one copy each instead of one per call site)
  __attribute__((noinline)) void alloc(long count) {
    release();
    T* q = nullptr;
    ATDN_HIP(hipMalloc(&q, (size_t)count * sizeof(T)));
    p = q; n = count;
    device_bytes_live += (long long)count * (long long)sizeof(T);
  }
  // Grows to at least `count` elements (contents are not kept). True when it allocated: the old address is gone.
  bool reserve(long count) {
    if (n >= count) return false;
    alloc(count);
    return true;
  }
  // hipFree waits for the work in flight on the block's device.
  __attribute__((noinline)) void release() {
    if (p) (void)hipFree(p);
    device_bytes_live -= (long long)n * (long long)sizeof(T);
    p = nullptr; n = 0;
  }
};

using DeviceBuf = DeviceArray<float>;
static_assert(!std::is_copy_constructible<DeviceBuf>::value, "a copy would be a second owner of the same block");

}  // namespace atdn
