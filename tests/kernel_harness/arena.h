// arena.h — what the entry points of harness.hip, rec_harness.hip and ctc_harness.hip share: one stream and the device buffers of a call,
// freed when the call returns; the first HIP error sticks and becomes the call's return value.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

namespace {

struct Arena {
  std::vector<void*> ptrs;
  hipError_t err = hipSuccess;
  hipStream_t st = nullptr;
  Arena() { chk(hipStreamCreateWithFlags(&st, hipStreamNonBlocking)); }
  ~Arena() {
    for (void* p : ptrs) (void)hipFree(p);
    if (st) (void)hipStreamDestroy(st);
  }
  bool chk(hipError_t e) {
    if (err == hipSuccess && e != hipSuccess) err = e;
    return err == hipSuccess;
  }
  void* raw(size_t bytes) {
    void* p = nullptr;
    if (!chk(hipMalloc(&p, bytes ? bytes : 16))) return nullptr;
    ptrs.push_back(p);
    return p;
  }
  template <class T> T* up(const T* host, size_t n) {       // NULL stays NULL
    if (!host) return nullptr;
    T* p = static_cast<T*>(raw(n * sizeof(T)));
    if (p && n) chk(hipMemcpyAsync(p, host, n * sizeof(T), hipMemcpyHostToDevice, st));
    return p;
  }
  template <class T> T* filled(size_t n, int byte) {
    T* p = static_cast<T*>(raw(n * sizeof(T)));
    if (p && n) chk(hipMemsetAsync(p, byte, n * sizeof(T), st));
    return p;
  }
  template <class T> void down(T* host, const T* dev, size_t n) {
    if (host && dev && n && err == hipSuccess) chk(hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, st));
  }
  int finish() {
    chk(hipGetLastError());
    chk(hipStreamSynchronize(st));
    return (int)err;
  }
};

size_t rup(size_t x, size_t m) { return (x + m - 1) / m * m; }

}  // namespace
