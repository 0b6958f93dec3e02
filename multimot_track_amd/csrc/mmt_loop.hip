// multimot_track_amd/csrc/mmt_loop.hip -- the device store of keyframe BoW vectors and
// k_loop_score, the data-parallel core of KeyFrameDatabase::DetectLoopCandidates
// (KeyFrameDatabase.cc:76-197) and of DetectLoop's minScore pass (LoopClosing.cc:127-144).
//
// k_loop_score: one wave per stored vector, kLoopWavesPerWG waves per workgroup.  The query's
// values and words are staged once per workgroup in dynamic LDS (12 bytes per word).  A step takes
// 64 consecutive stored words, one per lane; each lane binary-searches the query for its word.  A
// ballot gives the hits; their terms are packed in lane order into the wave's LDS row, and one
// running double, the same in every lane, is advanced over them.  Both lists ascend, so lane
// order within a step and step order are word
// order: the sum is Vocabulary::score's sequential loop (mmt_bow.hip) bit for bit, with serial
// work of the common words only.  No tree or shuffle reduction anywhere; -ffp-contract=off keeps
// the L2 product rounded apart from the add.
#include "mmt_loop.h"

#include <climits>

namespace mmt {

__global__ __launch_bounds__(64 * kLoopWavesPerWG) void k_loop_score(
    const uint32_t* __restrict__ words, const double* __restrict__ values,
    const LoopSlotDev* __restrict__ slots, int n_stored, int q_slot, int scoring,
    LoopScore* __restrict__ out) {
  extern __shared__ double lds_q[];
  const LoopSlotDev q = slots[q_slot];
  const int qn = q.len;
  double* row = lds_q + 64 * (threadIdx.x >> 6);  // this wave's 64 terms
  double* qv = lds_q + 64 * kLoopWavesPerWG;
  uint32_t* qw = reinterpret_cast<uint32_t*>(qv + qn);
  for (int i = threadIdx.x; i < qn; i += blockDim.x) {
    qv[i] = values[q.off + i];
    qw[i] = words[q.off + i];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * kLoopWavesPerWG + (threadIdx.x >> 6);
  if (k >= n_stored) return;
  const LoopSlotDev st = slots[k];
  double s = 0.0;
  int common = 0, first = INT_MAX;
  // the next step's word and value are loaded while this step searches
  uint32_t w_next = 0;
  double v_next = 0.0;
  if (lane < st.len) {
    w_next = words[st.off + lane];
    v_next = values[st.off + lane];
  }
  for (int base = 0; base < st.len; base += 64) {
    const int i = base + lane;
    const uint32_t w = w_next;
    const double wi = v_next;
    if (i + 64 < st.len) {
      w_next = words[st.off + i + 64];
      v_next = values[st.off + i + 64];
    }
    bool hit = false;
    int qi = 0;
    double term = 0.0;
    if (i < st.len) {
      int lo = 0, hi = qn;  // lower_bound of w in the query
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (qw[mid] < w) lo = mid + 1;
        else hi = mid;
      }
      qi = lo;
      hit = lo < qn && qw[lo] == w;
      if (hit) {
        const double vi = qv[lo];
        term = scoring == 1 ? vi * wi : fabs(vi - wi) - fabs(vi) - fabs(wi);
      }
    }
    const unsigned long long m = __ballot(hit);
    if (m == 0) continue;
    if (first == INT_MAX) first = __shfl(qi, __ffsll(m) - 1);
    const int nhit = __popcll(m);
    common += nhit;
    // the hits' terms packed in lane (= word) order into the wave's LDS row, then added one after
    // the other: the reads do not depend on the sum, so the chain is the adds alone.  One wave
    // writes and reads its row in program order; the fences keep the compiler from moving the
    // LDS accesses across each other.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    if (hit) row[__popcll(m & ((1ull << lane) - 1))] = term;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    for (int j = 0; j < nhit; j++) s += row[j];
  }
  if (lane == 0) {
    LoopScore r;
    r.common = common;
    r.first = first;
    r.sum = s;
    out[k] = r;
  }
}

LoopStore::~LoopStore() { release(); }

void LoopStore::release() {
  (void)hipFree(d_word_);
  (void)hipFree(d_value_);
  (void)hipFree(d_slot_);
  (void)hipFree(d_out_);
  d_word_ = nullptr;
  d_value_ = nullptr;
  d_slot_ = nullptr;
  d_out_ = nullptr;
  word_cap_ = value_cap_ = slot_cap_ = out_cap_ = 0;
}

void LoopStore::reset() {
  release();
  table.clear();
  used_ = 0;
  word_grown_ = value_grown_ = 0;
}

// Room for `need` elements: the capacity doubles (from first_cap) and the `used` elements in use
// are copied on the stream; the old array is freed once the copy is done.
template <typename T>
void LoopStore::grow(T** p, size_t& cap, size_t used, size_t need, size_t first_cap, int* grown,
                     hipStream_t s) {
  if (need <= cap) return;
  size_t ncap = cap ? cap : first_cap;
  while (ncap < need) ncap *= 2;
  T* np = nullptr;
  MMT_HIP(hipMalloc((void**)&np, ncap * sizeof(T)));
  if (*p && used > 0) {
    const hipError_t e = hipMemcpyAsync(np, *p, used * sizeof(T), hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) {
      (void)hipFree(np);
      throw DeviceError(std::string("LoopStore: copy to the grown array: ") + hipGetErrorString(e));
    }
  }
  const hipError_t e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    (void)hipFree(np);
    throw DeviceError(std::string("LoopStore: growing: ") + hipGetErrorString(e));
  }
  if (*p) {
    (void)hipFree(*p);
    if (grown) ++*grown;
  }
  *p = np;
  cap = ncap;
}

void LoopStore::set_bow(int32_t kf_id, const mmt_bow_vector& v, hipStream_t s) {
  if (kf_id < 0) throw ArgError("mmt_loop_set_bow: negative keyframe id");
  if (table.find(kf_id) >= 0)
    throw ArgError("mmt_loop_set_bow: keyframe " + std::to_string(kf_id) + " has a vector already");
  if (v.n < 0 || v.n > MMT_LOOP_MAX_WORDS)
    throw ArgError("mmt_loop_set_bow: word count outside [0, " +
                   std::to_string(MMT_LOOP_MAX_WORDS) + "]");
  if (v.n > 0 && (!v.word || !v.value)) throw ArgError("mmt_loop_set_bow: null vector arrays");
  for (int i = 1; i < v.n; i++)
    if (v.word[i] <= v.word[i - 1])
      throw ArgError("mmt_loop_set_bow: words are not strictly ascending");
  const size_t n = (size_t)v.n, ns = table.slots.size();
  constexpr size_t kFirstCap = 1 << 14;
  grow(&d_word_, word_cap_, used_, used_ + n, kFirstCap, &word_grown_, s);
  grow(&d_value_, value_cap_, used_, used_ + n, kFirstCap, &value_grown_, s);
  grow(&d_slot_, slot_cap_, ns, ns + 1, 256, nullptr, s);
  LoopSlotDev sd;
  sd.off = used_;
  sd.len = v.n;
  sd.pad = 0;
  if (n > 0) {
    MMT_HIP(hipMemcpyAsync(d_word_ + used_, v.word, n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    MMT_HIP(hipMemcpyAsync(d_value_ + used_, v.value, n * sizeof(double), hipMemcpyHostToDevice, s));
  }
  MMT_HIP(hipMemcpyAsync(d_slot_ + ns, &sd, sizeof(sd), hipMemcpyHostToDevice, s));
  MMT_HIP(hipStreamSynchronize(s));  // the caller's arrays and sd are read by now
  LoopSlot L;
  L.kf_id = kf_id;
  L.len = v.n;
  L.off = used_;
  table.slots.push_back(L);
  table.index[kf_id] = (int32_t)ns;
  used_ += n;
}

const std::vector<LoopScore>& LoopStore::score(int32_t kf_id, int scoring, hipStream_t s) {
  const int q = table.find(kf_id);
  if (q < 0) throw ArgError("keyframe " + std::to_string(kf_id) + " has no stored vector");
  const int ns = (int)table.slots.size();
  size_t ocap = out_cap_;
  if ((size_t)ns > out_cap_) {  // nothing to keep: free, then allocate
    (void)hipFree(d_out_);
    d_out_ = nullptr;
    out_cap_ = 0;
    size_t ncap = ocap ? ocap : 256;
    while (ncap < (size_t)ns) ncap *= 2;
    MMT_HIP(hipMalloc((void**)&d_out_, ncap * sizeof(LoopScore)));
    out_cap_ = ncap;
  }
  constexpr size_t kRowLds = sizeof(double) * 64 * kLoopWavesPerWG;  // the waves' term rows
  constexpr size_t kMaxLds = kRowLds + (size_t)MMT_LOOP_MAX_WORDS * 12;
  if (lds_set_ != kMaxLds) {
    MMT_HIP(hipFuncSetAttribute((const void*)k_loop_score,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds));
    lds_set_ = kMaxLds;
  }
  const size_t lds = kRowLds + (size_t)table.slots[q].len * 12;
  const int nwg = (ns + kLoopWavesPerWG - 1) / kLoopWavesPerWG;
  hipLaunchKernelGGL(k_loop_score, dim3(nwg), dim3(64 * kLoopWavesPerWG), lds, s, d_word_,
                     d_value_, d_slot_, ns, q, scoring, d_out_);
  MMT_HIP(hipGetLastError());
  h_out_.resize((size_t)ns);
  MMT_HIP(hipMemcpyAsync(h_out_.data(), d_out_, (size_t)ns * sizeof(LoopScore),
                         hipMemcpyDeviceToHost, s));
  MMT_HIP(hipStreamSynchronize(s));
  return h_out_;
}

void LoopStore::stats(mmt_loop_store_stats& out) const {
  out.n_stored = (int32_t)table.slots.size();
  out.n_members = table.n_members;
  out.word_capacity = (int64_t)word_cap_;
  out.value_capacity = (int64_t)value_cap_;
  out.word_grown = word_grown_;
  out.value_grown = value_grown_;
}

}  // namespace mmt
