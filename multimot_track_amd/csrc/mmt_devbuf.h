// multimot_track_amd/csrc/mmt_devbuf.h -- the scoped device allocation of the entry points that
// allocate per call (the C-ABI probes, the PnP / Sim3 solvers, vocabulary training).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "mmt_internal.h"

namespace mmt {

// n elements of T on the device (one when n is 0, so p is never null), freed at the end of the
// scope.  The copies count elements of T, not bytes; a zero count copies nothing.  up / down queue
// the copy on the stream: the host memory must stay alive until the stream is synchronised.
// up_now / down_now return when the copy is done.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;  // elements allocated
  explicit DevBuf(size_t n_) : n(std::max<size_t>(n_, 1)) {
    MMT_HIP(hipMalloc((void**)&p, n * sizeof(T)));
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { (void)hipFree(p); }

  void up(const T* h, size_t count, hipStream_t s, size_t first = 0) {
    if (!in_range(first, count)) return;
    MMT_HIP(hipMemcpyAsync(p + first, h, count * sizeof(T), hipMemcpyHostToDevice, s));
  }
  void up(const std::vector<T>& h, hipStream_t s) { up(h.data(), h.size(), s); }
  void up_now(const T* h, size_t count) {
    if (!in_range(0, count)) return;
    MMT_HIP(hipMemcpy(p, h, count * sizeof(T), hipMemcpyHostToDevice));
  }
  void down(T* h, size_t count, hipStream_t s, size_t first = 0) const {
    if (!in_range(first, count)) return;
    MMT_HIP(hipMemcpyAsync(h, p + first, count * sizeof(T), hipMemcpyDeviceToHost, s));
  }
  void down_now(T* h, size_t count, size_t first = 0) const {
    if (!in_range(first, count)) return;
    MMT_HIP(hipMemcpy(h, p + first, count * sizeof(T), hipMemcpyDeviceToHost));
  }

 private:
  // false: nothing to copy; a range past the allocation is the caller's bug
  bool in_range(size_t first, size_t count) const {
    if (first > n || count > n - first) throw DeviceError("DevBuf: copy outside the allocation");
    return count > 0;
  }
};

}  // namespace mmt
