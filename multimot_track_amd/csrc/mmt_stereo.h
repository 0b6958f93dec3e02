// multimot_track_amd/csrc/mmt_stereo.h -- stereo keypoint depth (Frame::ComputeStereoMatches,
// reference src/Frame.cc:849-1038) on the device: row table, Hamming search, SAD window with the
// sub-pixel parabola, median filter.  See mmt_stereo.hip for the semantics and the pins.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mmt.h"

namespace mmt {

constexpr int kStereoMaxLevels = 16;  // mmt_create accepts orb_nlevels <= 16

// Pyramid geometry and scale tables as the kernels read them (passed by value).
struct StereoLevels {
  int nlevels;
  int rows, cols;  // level 0
  int w[kStereoMaxLevels], h[kStereoMaxLevels], off[kStereoMaxLevels];
  float scale[kStereoMaxLevels], invScale[kStereoMaxLevels];
};

// One side of a pair on the device: its pyramid (the ORB engine's layout: level l at off[l], rows
// of w[l] bytes), keys, descriptors (n x 32) and the device word holding the key count.
struct StereoSide {
  const uint8_t* pyr;
  const mmt_kp* kps;
  const uint8_t* desc;
  const int* n;
};

// Workspace and outputs of the matcher, kept across calls.  Every launch goes on the caller's
// stream; nothing here synchronises.
class StereoMatcher {
 public:
  StereoMatcher() = default;
  ~StereoMatcher();
  StereoMatcher(const StereoMatcher&) = delete;
  StereoMatcher& operator=(const StereoMatcher&) = delete;
  // Rows of the image, keys per side at most (<= 16384), and the largest scale factor (bounds the
  // rows a right key is listed in).
  void ensure(int rows, int cap, float max_scale);
  // Row table, matcher, median stage for the left keys against the right ones; cap_l / cap_r bound
  // the device counts (they size the grids).  Outputs below hold cap_l entries.
  void run(const StereoLevels& lv, const StereoSide& left, const StereoSide& right, int cap_l,
           int cap_r, float bf, hipStream_t stream);
  // vSemLabel (Frame.cc:116-124): sem[i] = mask[(int)y * w + (int)x] of the left keys.
  void sem_labels(const StereoSide& left, int cap_l, const int32_t* d_mask, int w, int h,
                  hipStream_t stream);
  float* uR = nullptr;            // mvuRight
  float* depth = nullptr;         // mvDepth
  int32_t* right_idx = nullptr;   // vDescIndex
  int32_t* best_dist = nullptr;   // coarse bestDist (-1: search not reached)
  int32_t* sad = nullptr;         // window search's bestDist (-1: not reached)
  int32_t* sem = nullptr;         // vSemLabel
  mmt_stereo_counters* counters = nullptr;

 private:
  void release();
  int rows_ = 0, cap_ = 0, entries_ = 0;
  int* row_cnt_ = nullptr;    // rows: keys listed in the row, then the fill cursor
  int* row_start_ = nullptr;  // rows + 1
  int* row_idx_ = nullptr;    // entries_
  int32_t* acc_ = nullptr;    // SAD of an accepted key, else -1 (the median stage's input)
  StereoLevels* lv_dev_ = nullptr;  // device copy of the level tables, uploaded when they change
  StereoLevels lv_host_{};
};

}  // namespace mmt
