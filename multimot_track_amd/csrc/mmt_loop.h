// multimot_track_amd/csrc/mmt_loop.h -- the device store of keyframe BoW vectors and k_loop_score
// (mmt_loop.hip): one launch scores a stored vector against every stored vector.  The host half
// of the detection is mmt_loopdetect.{h,cpp}.
#pragma once
#include <vector>

#include "mmt_internal.h"
#include "mmt_loopdetect.h"

namespace mmt {

constexpr int kLoopWavesPerWG = 4;  // one wave per stored vector, 256 threads per workgroup

// one stored vector as the kernel reads it (16 bytes)
struct LoopSlotDev {
  uint64_t off;
  int32_t len;
  int32_t pad;
};

// Per-context store: one growing uint32 word array and one growing double value array (words
// ascending within a vector, as BowVecH), a device copy of (offset, length) per stored vector and
// the result records.  The arrays grow by reallocating and copying on the stream, doubling; a
// stored vector never changes.
class LoopStore {
 public:
  LoopStore() = default;
  LoopStore(const LoopStore&) = delete;
  LoopStore& operator=(const LoopStore&) = delete;
  ~LoopStore();

  void reset();
  // throws ArgError: a second vector for kf_id, n outside [0, MMT_LOOP_MAX_WORDS], words not
  // strictly ascending
  void set_bow(int32_t kf_id, const mmt_bow_vector& v, hipStream_t s);
  // one launch, one read-back, one synchronisation: a record per stored vector against kf_id's
  const std::vector<LoopScore>& score(int32_t kf_id, int scoring, hipStream_t s);

  LoopSlotTable table;
  void stats(mmt_loop_store_stats& out) const;

 private:
  void release();
  template <typename T>
  static void grow(T** p, size_t& cap, size_t used, size_t need, size_t first_cap, int* grown,
                   hipStream_t s);
  uint32_t* d_word_ = nullptr;
  double* d_value_ = nullptr;
  LoopSlotDev* d_slot_ = nullptr;
  LoopScore* d_out_ = nullptr;
  size_t word_cap_ = 0, value_cap_ = 0, slot_cap_ = 0, out_cap_ = 0;
  size_t used_ = 0;  // elements of the word / value arrays in use
  int word_grown_ = 0, value_grown_ = 0;
  size_t lds_set_ = 0;  // dynamic LDS the kernel has been allowed so far
  std::vector<LoopScore> h_out_;
};

}  // namespace mmt
