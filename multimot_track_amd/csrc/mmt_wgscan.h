// multimot_track_amd/csrc/mmt_wgscan.h -- integer scans and the order-preserving compaction of a
// workgroup (blockDim a multiple of 64; every thread of the workgroup calls them).  `s_w` is LDS,
// one int per wave.
#pragma once
#include <hip/hip_runtime.h>

namespace mmt {

// inclusive scan of v over the wave, in lane order
template <typename T>
__device__ __forceinline__ T wave_scan_incl(T v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T y = __shfl_up(v, o, 64);
    if (lane >= o) v += y;
  }
  return v;
}

// exclusive block-wide scan of one int per thread (thread order); returns the total
__device__ __forceinline__ int block_scan_excl(int v, int* s_w, int& excl) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int x = wave_scan_incl(v);
  if (lane == 63) s_w[wave] = x;
  __syncthreads();
  int off = 0, tot = 0;
  for (int w = 0; w < nw; w++) {
    const int c = s_w[w];
    if (w < wave) off += c;
    tot += c;
  }
  excl = off + x - v;
  __syncthreads();
  return tot;
}

// order-preserving compaction of one flag per thread: returns this thread's slot (or -1) and
// advances `base` by the round's total.  NW: the workgroup's wave count (blockDim = 64 NW), known
// to the kernel, so the loop over the waves unrolls
template <int NW>
__device__ __forceinline__ int wg_compact_slot(bool keep, int* s_w, int& base) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(keep);
  if (lane == 0) s_w[wave] = __popcll(bal);
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < NW; w++) {
    const int c = s_w[w];
    if (w < wave) off += c;
    tot += c;
  }
  const int slot = keep ? base + off + __popcll(bal & ((1ull << lane) - 1ull)) : -1;
  base += tot;
  __syncthreads();
  return slot;
}

}  // namespace mmt
