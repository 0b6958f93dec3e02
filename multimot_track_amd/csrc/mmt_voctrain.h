// multimot_track_amd/csrc/mmt_voctrain.h -- DBoW2's vocabulary training on the GPU:
// TemplatedVocabulary::create(training_features, k, L, weighting, scoring).
//
// Reference: Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:558-587 (create), 642-819 (HKmeansStep),
// 833-913 (initiateClustersKMpp), 918-996 (createWords, setNodeWeights); FORB.cpp:28-101
// (meanValue, distance); DUtils/Random.h (RandomInt, RandomValue).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mmt.h"
#include "mmt_bow.h"

namespace mmt {

// the pinned random stream: splitmix64's output function
inline uint64_t voc_mix(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// create(): desc is image_start[n_images] x 32 bytes on the host.  Fills `out` (tree, words,
// weights in full precision) and `stats`; throws ArgError / DeviceError.
void train_vocabulary(const uint8_t* desc, const int32_t* image_start, int n_images,
                      const mmt_voc_train_params& p, Vocabulary& out, mmt_voc_train_stats& stats,
                      hipStream_t st);

}  // namespace mmt
