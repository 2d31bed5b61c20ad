// mcl_buffer.h -- the one owner of a device or pinned-host allocation: the pointer and its capacity in one object, so
// that they cannot disagree.  Device-free (no HIP header: tests/host_san/host_pure_driver.cpp drives it under the host
// sanitizers with an allocator that fails on command); the two allocators of the library are in mcl_device.h.
//   Alloc::alloc(void** p, size_t bytes) -> MCL_OK, MCL_ERR_ALLOC (out of memory) or MCL_ERR_HIP;  Alloc::release(void* p)
#pragma once
#include <cstddef>

#include "../../include/mcl.h"

template <class T, class Alloc>
struct Buffer {
  T* p = nullptr;
  size_t cap = 0;   // elements

  Buffer() = default;
  Buffer(const Buffer&) = delete;
  Buffer& operator=(const Buffer&) = delete;
  Buffer(Buffer&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  Buffer& operator=(Buffer&& o) noexcept {
    if (this != &o) {
      reset();
      p = o.p, cap = o.cap;
      o.p = nullptr, o.cap = 0;
    }
    return *this;
  }
  ~Buffer() { reset(); }

  // (kernel argument blocks, pointer arithmetic and `if (!buf)` read as they do with a raw pointer)
  operator T*() const { return p; }

  void reset() {
    if (p) Alloc::release(p);
    p = nullptr;
    cap = 0;
  }
  // Room for `count` elements.  Within the capacity: nothing happens.  Otherwise the old block is freed FIRST (the
  // contents are not kept) and {p, cap} are committed only when the new one exists: a failure leaves {nullptr, 0}.
  int reserve(size_t count) {
    if (count <= cap) return MCL_OK;
    reset();
    void* q = nullptr;
    const int rc = Alloc::alloc(&q, sizeof(T) * count);
    if (rc != MCL_OK) return rc;
    p = static_cast<T*>(q);
    cap = count;
    return MCL_OK;
  }
};
