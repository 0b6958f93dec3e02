// multimot_track_amd/csrc/mmt_loopdetect.h -- the host half of loop detection:
// KeyFrameDatabase::DetectLoopCandidates (KeyFrameDatabase.cc:76-197) and LoopClosing::DetectLoop
// (LoopClosing.cc:105-231) over the per-keyframe triples k_loop_score (mmt_loop.hip) writes.
// Plain C++, no device headers: tests/loop_detect_host_check.cpp builds it alone.
//
// The reference reaches its numbers through an inverted file and three scratch fields per keyframe
// (mnLoopQuery, mnLoopWords, mLoopScore).  Here they are per-query arrays over the slot table:
//   lKFsSharingWords = the database members with common > 0 that are not connected to the query,
//                      sorted by (first, add sequence): the reference walks the query's words
//                      ascending and each word's list in insertion order, and erase keeps the
//                      others' relative order;
//   mnLoopQuery == id  <=> the keyframe is in that list (a connected keyframe never gets it);
//   mnLoopWords        = common;   mLoopScore = (float)score, set where common > minCommonWords.
// Nothing survives from one query to the next except the database and mvConsistentGroups.
//
// detect() returns the enough-consistent candidates.  The reference's own DetectLoop ends in
// `return false` in this fork (LoopClosing.cc:225, "oringinal is true"); what the caller does with
// a non-empty list is the caller's business.
#pragma once
#include <cstdint>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/mmt.h"

namespace mmt {

// k_loop_score's record for one stored vector (16 bytes, read back as written)
struct LoopScore {
  int32_t common;  // words in both vectors (mnLoopWords of a database member)
  int32_t first;   // query index of the lowest common word, INT_MAX without one
  double sum;      // the raw sum of DBoW2's scoring loop, added in ascending word order
};

struct LoopSlot {
  int32_t kf_id = -1;
  int32_t len = 0;
  uint64_t off = 0;   // first element in the store's word / value arrays
  uint64_t seq = 0;   // add sequence number (valid while member)
  bool member = false;
};

// stored vectors in storage order, and the database membership (KeyFrameDatabase::add / erase)
struct LoopSlotTable {
  std::vector<LoopSlot> slots;
  std::unordered_map<int32_t, int32_t> index;  // kf_id -> slot
  uint64_t next_seq = 0;
  int n_members = 0;

  void clear();
  int find(int32_t kf_id) const;  // -1: no stored vector
  // false: no stored vector / already a member
  bool db_add(int32_t kf_id);
  // erase of a non-member does nothing; false: no stored vector
  bool db_erase(int32_t kf_id);
};

// Vocabulary::score's last step (mmt_bow.hip): L1 -sum/2, L2 sum >= 1 ? 1 : 1 - sqrt(1 - sum)
double loop_finish_score(double sum, int scoring);

class LoopDetector {
 public:
  using Group = std::pair<std::vector<int32_t>, int>;  // sorted member ids, consistency counter

  void reset(int scoring);
  int scoring() const { return scoring_; }
  const std::vector<Group>& groups() const { return groups_; }
  const std::string& error() const { return err_; }

  // mnId < mLastLoopKFid + 10: detect() adds to the database and returns without reading scores
  static bool early_exit(int32_t kf_id, int32_t last_loop_kf_id) {
    return (int64_t)kf_id < (int64_t)last_loop_kf_id + 10;
  }

  // KeyFrameDatabase::DetectLoopCandidates(pKF, minScore).  sc: one record per slot of T, scored
  // against kf_id's vector.  false (and error()) on a bad argument.
  bool candidates(const LoopSlotTable& T, const LoopScore* sc, int32_t kf_id, float min_score,
                  const mmt_covis_graph& g, std::vector<int32_t>& out);

  // LoopClosing::DetectLoop for keyframe kf_id; sc may be null when early_exit() holds.  More than
  // max_out candidates is an error.  On an error neither T nor the groups have changed.
  bool detect(LoopSlotTable& T, const LoopScore* sc, int32_t kf_id, int32_t last_loop_kf_id,
              int consistency_th, const mmt_covis_graph& g, int max_out, mmt_loop_result& res,
              std::vector<int32_t>& cand, std::vector<int32_t>& enough);

 private:
  bool fail(const std::string& m) {
    err_ = m;
    return false;
  }
  bool check_graph(const mmt_covis_graph& g, int32_t kf_id);
  bool list_of(const mmt_covis_graph& g, const int32_t* start, const int32_t* list, int32_t id,
               const int32_t** b, const int32_t** e);
  int scoring_ = 0;
  std::vector<Group> groups_;  // mvConsistentGroups
  std::string err_;
};

}  // namespace mmt
