// multimot_track_amd/csrc/mmt_stereo.hip -- Frame::ComputeStereoMatches on gfx950 (reference
// src/Frame.cc:849-1038; this fork: maxD = 200, minD = 0, the vDescIndex output).
//
// Launch sequence, all on the caller's stream, no host round trip:
//   k_stereo_rows_count / _scan / _fill   vRowIndices as a CSR (:862-879).  The fill is unordered
//                                          (atomics): the search below does not depend on it.
//   k_stereo_match                         one wave per left key, four per workgroup
//   k_stereo_median                        one workgroup: rank selection and the clearing pass
//
// Semantics, in the reference's order (tests/stereo_ref_py.py restates them sequentially, the
// results are equal bit for bit: every decision is an integer or one float32 operation, compiled
// with -ffp-contract=off and the correctly rounded fp32 divide):
//   row table   right key iR is listed in rows floor(y - r) .. ceil(y + r), r = 1.2f * scale[octave]
//   search      left key reads row (int)vL; a candidate needs octave in [level - 1, level + 1] and
//               uL - 200 <= uR <= uL; the smallest Hamming distance below TH_HIGH = 100 wins under
//               a strict <, so the lowest iR wins ties: a wave-min over (dist << 16) | iR
//   vDescIndex  right_idx = bestIdxR only if bestIdxR != 0 (:943): right key 0 can win and be
//               refined, yet is reported as -1
//   refinement  only below thOrbDist = 75, at the left key's level: C round() of the float
//               products x * invScale, 11 x 11 windows of the unblurred pyramid minus their own
//               centre pixel, L1 distance for incR = -5 .. 5 ascending under a strict <; skipped
//               when scaleduR0 < 0 || scaleduR0 + 11 >= cols (:972) and when the best shift is
//               -5 or 5.  The sums are integers <= 121 * 510, exact in float.
//   parabola    deltaR = (d1 - d3) / (2.0f * (d1 + d3 - 2.0f * d2)); skipped outside [-1, 1]; a NaN
//               passes that test and fails the disparity range test
//   result      bestuR = scale * ((float)scaleduR0 + (float)bestincR + deltaR), disparity = uL -
//               bestuR accepted in [0, 200); exactly 0 becomes 0.01 with bestuR = uL - 0.01
//   median      thDist = 1.5f * 1.4f * median, median = element [size / 2] of the sorted accepted
//               SADs; every accepted key with (float)dist >= thDist is cleared (what the
//               reference's walk down the sorted list does), so a rank selection replaces the sort
//
// Pins where the reference is undefined:
//   (a) no accepted key: the reference reads vDistIdx[0] of an empty vector.  Nothing is cleared;
//       median = -1, th_dist = 0.
//   (b) scaleduR0 - 10 < 0 (OpenCV would throw in colRange; extractor keys cannot reach it, level
//       coordinates are >= 16): skipped like the border test and counted with it.
//   (c) keys the reference would index out of bounds with (a left window that leaves its level, a
//       right key whose rows leave [0, rows), an octave outside the pyramid) are refused by the
//       host entry point before any launch.  The kernels still guard every index: such a left key
//       counts as a window-edge skip, such rows are clipped.

#include "mmt_stereo.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#include "mmt_internal.h"

namespace mmt {
namespace {

constexpr int kThHigh = 100;     // ORBmatcher::TH_HIGH
constexpr int kThOrbDist = 75;   // (TH_HIGH + TH_LOW) / 2
constexpr int kW = 5, kL = 5;    // window half size, shift range
constexpr int kWinPx = (2 * kW + 1) * (2 * kW + 1);  // 121
constexpr int kStripW = 2 * (kW + kL) + 1;           // 21
constexpr int kStripPx = (2 * kW + 1) * kStripW;     // 231
constexpr int kWaves = 4;
constexpr int kSadMax = kWinPx * 510;

__device__ inline void row_range(const mmt_kp& k, const StereoLevels& lv, int& lo, int& hi) {
  const int o = min(max(k.octave, 0), lv.nlevels - 1);
  const float r = 1.2f * lv.scale[o];
  const float top = k.y + r, bot = k.y - r;
  hi = min((int)ceilf(top), lv.rows - 1);
  lo = max((int)floorf(bot), 0);
}

__global__ __launch_bounds__(256) void k_stereo_rows_count(const StereoLevels* __restrict__ lvp,
                                                           const mmt_kp* __restrict__ kr,
                                                           const int* __restrict__ d_nr,
                                                           int cap_r, int* __restrict__ row_cnt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= min(*d_nr, cap_r)) return;
  int lo, hi;
  row_range(kr[i], *lvp, lo, hi);
  for (int y = lo; y <= hi; y++) atomicAdd(&row_cnt[y], 1);
}

// One workgroup: row_start = exclusive scan of row_cnt; row_cnt is cleared (the fill's cursor).
__global__ __launch_bounds__(1024) void k_stereo_rows_scan(int* __restrict__ row_cnt, int rows,
                                                           int* __restrict__ row_start) {
  __shared__ int s[1024];
  const int tid = threadIdx.x;
  const int chunk = (rows + 1023) / 1024;
  const int b = min(tid * chunk, rows), e = min(b + chunk, rows);
  int sum = 0;
  for (int y = b; y < e; y++) sum += row_cnt[y];
  s[tid] = sum;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int v = tid >= o ? s[tid - o] : 0;
    __syncthreads();
    s[tid] += v;
    __syncthreads();
  }
  int run = s[tid] - sum;
  for (int y = b; y < e; y++) {
    const int c = row_cnt[y];
    row_start[y] = run;
    row_cnt[y] = 0;
    run += c;
  }
  if (tid == 1023) row_start[rows] = s[1023];
}

__global__ __launch_bounds__(256) void k_stereo_rows_fill(const StereoLevels* __restrict__ lvp,
                                                          const mmt_kp* __restrict__ kr,
                                                          const int* __restrict__ d_nr, int cap_r,
                                                          int* __restrict__ row_cur,
                                                          const int* __restrict__ row_start,
                                                          int* __restrict__ row_idx, int entries) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= min(*d_nr, cap_r)) return;
  int lo, hi;
  row_range(kr[i], *lvp, lo, hi);
  for (int y = lo; y <= hi; y++) {
    const int p = row_start[y] + atomicAdd(&row_cur[y], 1);
    if (p < entries) row_idx[p] = i;
  }
}

struct MatchArgs {
  const StereoLevels* lv;
  StereoSide l, r;
  int cap_l, cap_r, entries;
  const int* row_start;
  const int* row_idx;
  float* uR;
  float* depth;
  int32_t* right_idx;
  int32_t* best_dist;
  int32_t* sad;
  int32_t* acc;
  mmt_stereo_counters* c;
  float bf;
};

__global__ __launch_bounds__(64 * kWaves) void k_stereo_match(const MatchArgs a) {
  __shared__ int s_l[kWaves][128];
  __shared__ int s_r[kWaves][232];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int iL = blockIdx.x * kWaves + wave;
  const StereoLevels& lv = *a.lv;
  const int nl = min(*a.l.n, a.cap_l), nr = min(*a.r.n, a.cap_r);
  // everything below is uniform over the wave: each wave owns one left key
  const bool has = iL < nl;
  int level = 0, best_dist = -1, best_r = 0;
  int su = 0, sv = 0, sr0 = 0, lw = 0;
  float uL = 0.f;
  bool coarse = false, refine = false;
  if (has) {
    const mmt_kp k = a.l.kps[iL];
    level = k.octave;
    uL = k.x;
    const float vL = k.y;
    const int row = (int)vL;
    const float minU = uL - 200.f, maxU = uL - 0.f;
    if (level >= 0 && level < lv.nlevels && vL >= 0.f && row < lv.rows && !(maxU < 0.f)) {
      const int b = a.row_start[row], e = min(a.row_start[row + 1], a.entries);
      if (e > b) {
        uint32_t dl[8];
        const uint32_t* pd = (const uint32_t*)(a.l.desc + (size_t)32 * iL);
#pragma unroll
        for (int j = 0; j < 8; j++) dl[j] = pd[j];
        unsigned key = (unsigned)kThHigh << 16;  // bestDist = TH_HIGH, bestIdxR = 0
        for (int c = b + lane; c < e; c += 64) {
          const int iR = a.row_idx[c];
          if ((unsigned)iR >= (unsigned)nr) continue;
          const int oR = a.r.kps[iR].octave;
          const float xR = a.r.kps[iR].x;
          if (oR < level - 1 || oR > level + 1) continue;
          if (!(xR >= minU && xR <= maxU)) continue;
          const uint32_t* pr = (const uint32_t*)(a.r.desc + (size_t)32 * iR);
          int d = 0;
#pragma unroll
          for (int j = 0; j < 8; j++) d += __popc(dl[j] ^ pr[j]);
          if (d < kThHigh) key = min(key, ((unsigned)d << 16) | (unsigned)iR);
        }
        for (int o = 32; o > 0; o >>= 1) key = min(key, (unsigned)__shfl_xor((int)key, o, 64));
        best_dist = (int)(key >> 16);
        best_r = (int)(key & 0xffffu);
        if (best_dist < kThOrbDist) {
          coarse = true;
          const float s = lv.invScale[level];
          const float xr0 = a.r.kps[best_r].x;
          su = (int)roundf(uL * s);
          sv = (int)roundf(vL * s);
          sr0 = (int)roundf(xr0 * s);
          lw = lv.w[level];
          const int lh = lv.h[level];
          const bool edge = sr0 < 0 || sr0 + kL + kW + 1 >= lw || sr0 - kL - kW < 0 ||  // :972, (b)
                            su - kW < 0 || su + kW >= lw || sv - kW < 0 || sv + kW >= lh;
          refine = !edge;
        }
      }
    }
  }
  if (refine) {
    const uint8_t* pl = a.l.pyr + lv.off[level] + (size_t)(sv - kW) * lw + (su - kW);
    for (int p = lane; p < kWinPx; p += 64) s_l[wave][p] = pl[(p / 11) * lw + p % 11];
    const uint8_t* pr = a.r.pyr + lv.off[level] + (size_t)(sv - kW) * lw + (sr0 - kL - kW);
    for (int p = lane; p < kStripPx; p += 64) s_r[wave][p] = pr[(p / kStripW) * lw + p % kStripW];
  }
  __syncthreads();  // every wave reaches it: nothing above returns
  int sad = -1;
  float out_u = -1.f, out_z = -1.f;
  int stage = 0;  // 1 window edge, 2 end shift, 3 delta, 4 range, 5 accepted, 6 accepted + clamped
  if (coarse && !refine) stage = 1;
  if (refine) {
    int sum[2 * kL + 1];
#pragma unroll
    for (int j = 0; j <= 2 * kL; j++) sum[j] = 0;
    const int cl = s_l[wave][kW * 11 + kW];
    for (int p = lane; p < kWinPx; p += 64) {
      const int row = p / 11, col = p % 11;
      const int l = s_l[wave][p] - cl;
#pragma unroll
      for (int j = 0; j <= 2 * kL; j++) {  // incR = j - 5: strip column col + j, centre kW + j
        const int r = s_r[wave][row * kStripW + col + j] - s_r[wave][kW * kStripW + kW + j];
        sum[j] += abs(l - r);
      }
    }
#pragma unroll
    for (int j = 0; j <= 2 * kL; j++)
      for (int o = 32; o > 0; o >>= 1) sum[j] += __shfl_xor(sum[j], o, 64);
    int best = INT_MAX, bj = 0;
#pragma unroll
    for (int j = 0; j <= 2 * kL; j++)
      if (sum[j] < best) {
        best = sum[j];
        bj = j;
      }
    sad = best;
    if (bj == 0 || bj == 2 * kL) {
      stage = 2;
    } else {
      float d1 = 0.f, d2 = 0.f, d3 = 0.f;
#pragma unroll
      for (int j = 1; j < 2 * kL; j++)
        if (j == bj) {
          d1 = (float)sum[j - 1];
          d2 = (float)sum[j];
          d3 = (float)sum[j + 1];
        }
      const float delta = (d1 - d3) / (2.0f * (d1 + d3 - 2.0f * d2));
      if (delta < -1.f || delta > 1.f) {
        stage = 3;
      } else {
        float best_u = lv.scale[level] * ((float)sr0 + (float)(bj - kL) + delta);
        float disparity = uL - best_u;
        if (disparity >= 0.f && disparity < 200.f) {
          stage = 5;
          if (disparity <= 0.f) {
            disparity = (float)0.01;
            best_u = (float)((double)uL - 0.01);
            stage = 6;
          }
          out_z = a.bf / disparity;
          out_u = best_u;
        } else {
          stage = 4;
        }
      }
    }
  }
  if (has && lane == 0) {
    a.uR[iL] = out_u;
    a.depth[iL] = out_z;
    a.right_idx[iL] = best_r != 0 ? best_r : -1;
    a.best_dist[iL] = best_dist;
    a.sad[iL] = sad;
    a.acc[iL] = stage >= 5 ? sad : -1;
    if (coarse) atomicAdd(&a.c->n_coarse, 1);
    if (stage == 1) atomicAdd(&a.c->n_window_edge, 1);
    if (stage == 2) atomicAdd(&a.c->n_end_shift, 1);
    if (stage == 3) atomicAdd(&a.c->n_delta, 1);
    if (stage == 4) atomicAdd(&a.c->n_range, 1);
    if (stage == 6) atomicAdd(&a.c->n_clamped, 1);
  }
}

// cum = inclusive scan of hist[0..256) (all 1024 threads call it; ends synchronised).
__device__ inline void wg_scan_256(const int* hist, int* cum, int tid) {
  if (tid < 256) cum[tid] = hist[tid];
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int v = (tid < 256 && tid >= o) ? cum[tid - o] : 0;
    __syncthreads();
    if (tid < 256) cum[tid] += v;
    __syncthreads();
  }
}

// The bin that holds the element of rank k (0-based, ascending) and k's rank inside that bin; one
// thread writes, none when k is not below the total.
__device__ inline void find_rank(const int* hist, const int* cum, int tid, int k, int* bin,
                                 int* rank) {
  if (tid < 256) {
    const int incl = cum[tid], excl = incl - hist[tid];
    if (excl <= k && k < incl) {
      *bin = tid;
      *rank = k - excl;
    }
  }
}

// One workgroup.  The median of the accepted SADs (element [size / 2] in ascending order) by two
// LDS histograms (the high byte, then the low byte inside the selected bin), then the clearing pass.
__global__ __launch_bounds__(1024) void k_stereo_median(const int* __restrict__ d_nl, int cap_l,
                                                        const int32_t* __restrict__ acc,
                                                        float* __restrict__ uR,
                                                        float* __restrict__ depth,
                                                        int32_t* __restrict__ right_idx,
                                                        mmt_stereo_counters* __restrict__ c) {
  __shared__ int hist[256];
  __shared__ int cum[256];
  __shared__ int s_bin, s_rank, s_total, s_removed, s_low, s_rank2;
  const int tid = threadIdx.x;
  const int n = min(*d_nl, cap_l);
  if (tid < 256) hist[tid] = 0;
  if (tid == 0) s_removed = 0;
  __syncthreads();
  for (int i = tid; i < n; i += 1024) {
    const int v = acc[i];
    if (v >= 0) atomicAdd(&hist[min(v, kSadMax) >> 8], 1);
  }
  __syncthreads();
  wg_scan_256(hist, cum, tid);
  if (tid == 0) s_total = cum[255];
  __syncthreads();
  find_rank(hist, cum, tid, s_total / 2, &s_bin, &s_rank);
  __syncthreads();
  const int total = s_total, bin = s_bin;
  if (total == 0) {  // pin (a): nothing is cleared
    if (tid == 0) {
      c->n_accepted = 0;
      c->n_median_removed = 0;
      c->median = -1;
      c->th_dist = 0.f;
    }
    return;
  }
  if (tid < 256) hist[tid] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += 1024) {
    const int v = acc[i];
    if (v >= 0 && (min(v, kSadMax) >> 8) == bin) atomicAdd(&hist[v & 255], 1);
  }
  __syncthreads();
  wg_scan_256(hist, cum, tid);
  find_rank(hist, cum, tid, s_rank, &s_low, &s_rank2);
  __syncthreads();
  const int median = (bin << 8) | s_low;
  const float th = 1.5f * 1.4f * (float)median;
  for (int i = tid; i < n; i += 1024) {
    const int v = acc[i];
    if (v >= 0 && (float)v >= th) {
      uR[i] = -1.f;
      depth[i] = -1.f;
      right_idx[i] = -1;
      atomicAdd(&s_removed, 1);
    }
  }
  __syncthreads();
  if (tid == 0) {
    c->n_accepted = total;
    c->n_median_removed = s_removed;
    c->median = median;
    c->th_dist = th;
  }
}

__global__ __launch_bounds__(256) void k_stereo_sem(const mmt_kp* __restrict__ kl,
                                                    const int* __restrict__ d_nl, int cap_l,
                                                    const int32_t* __restrict__ mask, int w, int h,
                                                    int32_t* __restrict__ sem) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= min(*d_nl, cap_l)) return;
  const int u = (int)kl[i].x, v = (int)kl[i].y;  // :120-123
  sem[i] = (u >= 0 && u < w && v >= 0 && v < h) ? mask[(size_t)v * w + u] : 0;
}

}  // namespace

StereoMatcher::~StereoMatcher() { release(); }

void StereoMatcher::release() {
  void* ptrs[] = {uR, depth, right_idx, best_dist, sad, sem, counters, row_cnt_, row_start_,
                  row_idx_, acc_, lv_dev_};
  for (void* p : ptrs) (void)hipFree(p);
  uR = depth = nullptr;
  right_idx = best_dist = sad = sem = acc_ = nullptr;
  counters = nullptr;
  row_cnt_ = row_start_ = row_idx_ = nullptr;
  lv_dev_ = nullptr;
  rows_ = cap_ = entries_ = 0;
}

void StereoMatcher::ensure(int rows, int cap, float max_scale) {
  // a right key is listed in at most 2 r + 3 rows, r = 1.2 * its scale factor
  const int per_key = (int)std::ceil(2.0 * 1.2 * (double)max_scale) + 4;
  if (rows <= rows_ && cap <= cap_ && cap * per_key <= entries_) return;
  rows = std::max(rows, rows_);  // grow only
  cap = std::max(cap, cap_);
  const int entries = std::max(cap * per_key, entries_);
  release();
  const size_t c = (size_t)std::max(cap, 1);
  MMT_HIP(hipMalloc((void**)&uR, c * sizeof(float)));
  MMT_HIP(hipMalloc((void**)&depth, c * sizeof(float)));
  MMT_HIP(hipMalloc((void**)&right_idx, c * sizeof(int32_t)));
  MMT_HIP(hipMalloc((void**)&best_dist, c * sizeof(int32_t)));
  MMT_HIP(hipMalloc((void**)&sad, c * sizeof(int32_t)));
  MMT_HIP(hipMalloc((void**)&sem, c * sizeof(int32_t)));
  MMT_HIP(hipMalloc((void**)&acc_, c * sizeof(int32_t)));
  MMT_HIP(hipMalloc((void**)&counters, sizeof(mmt_stereo_counters)));
  MMT_HIP(hipMalloc((void**)&row_cnt_, (size_t)rows * sizeof(int)));
  MMT_HIP(hipMalloc((void**)&row_start_, ((size_t)rows + 1) * sizeof(int)));
  MMT_HIP(hipMalloc((void**)&row_idx_, (size_t)std::max(entries, 1) * sizeof(int)));
  MMT_HIP(hipMalloc((void**)&lv_dev_, sizeof(StereoLevels)));
  memset(&lv_host_, 0xff, sizeof(lv_host_));
  rows_ = rows;
  cap_ = cap;
  entries_ = entries;
}

void StereoMatcher::run(const StereoLevels& lv, const StereoSide& left, const StereoSide& right,
                        int cap_l, int cap_r, float bf, hipStream_t stream) {
  if (lv.rows > rows_ || cap_l > cap_ || cap_r > cap_) throw ArgError("stereo workspace too small");
  if (memcmp(&lv, &lv_host_, sizeof(lv)) != 0) {  // once per context in practice
    MMT_HIP(hipStreamSynchronize(stream));
    MMT_HIP(hipMemcpy(lv_dev_, &lv, sizeof(lv), hipMemcpyHostToDevice));
    lv_host_ = lv;
  }
  MMT_HIP(hipMemsetAsync(row_cnt_, 0, (size_t)lv.rows * sizeof(int), stream));
  MMT_HIP(hipMemsetAsync(counters, 0, sizeof(mmt_stereo_counters), stream));
  const int gr = (std::max(cap_r, 1) + 255) / 256;
  hipLaunchKernelGGL(k_stereo_rows_count, dim3(gr), dim3(256), 0, stream, lv_dev_, right.kps,
                     right.n, cap_r, row_cnt_);
  hipLaunchKernelGGL(k_stereo_rows_scan, dim3(1), dim3(1024), 0, stream, row_cnt_, lv.rows,
                     row_start_);
  hipLaunchKernelGGL(k_stereo_rows_fill, dim3(gr), dim3(256), 0, stream, lv_dev_, right.kps,
                     right.n, cap_r, row_cnt_, row_start_, row_idx_, entries_);
  MatchArgs a;
  a.lv = lv_dev_;
  a.l = left;
  a.r = right;
  a.cap_l = cap_l;
  a.cap_r = cap_r;
  a.entries = entries_;
  a.row_start = row_start_;
  a.row_idx = row_idx_;
  a.uR = uR;
  a.depth = depth;
  a.right_idx = right_idx;
  a.best_dist = best_dist;
  a.sad = sad;
  a.acc = acc_;
  a.c = counters;
  a.bf = bf;
  hipLaunchKernelGGL(k_stereo_match, dim3((std::max(cap_l, 1) + kWaves - 1) / kWaves),
                     dim3(64 * kWaves), 0, stream, a);
  hipLaunchKernelGGL(k_stereo_median, dim3(1), dim3(1024), 0, stream, left.n, cap_l, acc_, uR,
                     depth, right_idx, counters);
  MMT_HIP(hipGetLastError());
}

void StereoMatcher::sem_labels(const StereoSide& left, int cap_l, const int32_t* d_mask, int w,
                               int h, hipStream_t stream) {
  if (cap_l > cap_) throw ArgError("stereo workspace too small");
  hipLaunchKernelGGL(k_stereo_sem, dim3((std::max(cap_l, 1) + 255) / 256), dim3(256), 0, stream,
                     left.kps, left.n, cap_l, d_mask, w, h, sem);
  MMT_HIP(hipGetLastError());
}

}  // namespace mmt
