// multimot_track_amd/csrc/mmt_bowvec.h -- DBoW2's per-image vectors as the host keeps them (plain
// C++: the map graph holds them and is compiled without the device headers).
#pragma once
#include <cstdint>
#include <vector>

namespace mmt {

// DBoW2::BowVector (std::map<WordId, WordValue>) and FeatureVector (std::map<NodeId,
// std::vector<unsigned int>>) as flat arrays (words / nodes ascending)
struct BowVecH {
  std::vector<uint32_t> word;
  std::vector<double> value;
};
struct FeatVecH {
  std::vector<uint32_t> node;
  std::vector<int> start{0};
  std::vector<int> feat;
};

}  // namespace mmt
