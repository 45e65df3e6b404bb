// shim_stage.h -- staging for the per-call RTCD shims (host pointers): every
// shim carves its device buffers out of the per-thread scratch through one
// Stage and copies through it on the shim stream.
#pragma once
#include "lavish_internal.h"

namespace lavish {

// bump allocator over the per-thread scratch for one shim call
struct Stage {
  char* base;
  size_t cap, used = 0;
  hipStream_t s;
  // cap: at least the sum of pad() over the pieces the call takes
  explicit Stage(size_t cap) : base((char*)shim_scratch(cap)), cap(cap), s(shim_stream()) {}
  static constexpr size_t pad(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
  void* take(size_t bytes) {
    void* p = base + used;
    used += pad(bytes);
    if (used > cap) set_error("shim stage overflow", hipErrorOutOfMemory, __FILE__, __LINE__);
    return p;
  }
  template <typename T>
  T* take_n(size_t n) {
    return (T*)take(n * sizeof(T));
  }
  // copy a w x h window (stride in elements) into a compact device block
  template <typename T>
  T* block(const T* host, ptrdiff_t stride, int w, int h) {
    T* d = take_n<T>((size_t)w * h);
    LAVISH_CHECK(hipMemcpy2DAsync(d, (size_t)w * sizeof(T), host, (size_t)stride * sizeof(T),
                                  (size_t)w * sizeof(T), h, hipMemcpyHostToDevice, s));
    return d;
  }
  // and a compact device block back into the caller's window
  template <typename T>
  void block_out(T* host, ptrdiff_t stride, const T* dev, int w, int h) {
    LAVISH_CHECK(hipMemcpy2DAsync(host, (size_t)stride * sizeof(T), dev, (size_t)w * sizeof(T),
                                  (size_t)w * sizeof(T), h, hipMemcpyDeviceToHost, s));
  }
  template <typename T>
  T* copy_in(const T* host, size_t n) {
    T* d = take_n<T>(n);
    LAVISH_CHECK(hipMemcpyAsync(d, host, n * sizeof(T), hipMemcpyHostToDevice, s));
    return d;
  }
  template <typename T>
  void copy_out(T* host, const T* dev, size_t n) {
    LAVISH_CHECK(hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, s));
  }
  void sync() { LAVISH_CHECK(hipStreamSynchronize(s)); }
};

constexpr size_t kStageCap = 4u << 20;  // 128x128 u16 x (src + 4 refs + second) + outputs

inline void must(int rc, const char* what) {
  if (rc != 0) shim_reject(what, rc);
}

}  // namespace lavish
