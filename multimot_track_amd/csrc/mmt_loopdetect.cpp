// multimot_track_amd/csrc/mmt_loopdetect.cpp -- KeyFrameDatabase::DetectLoopCandidates and
// LoopClosing::DetectLoop on the host (see mmt_loopdetect.h).  Plain C++.
#include "mmt_loopdetect.h"

#include <algorithm>
#include <climits>
#include <cmath>

namespace mmt {

void LoopSlotTable::clear() {
  slots.clear();
  index.clear();
  next_seq = 0;
  n_members = 0;
}

int LoopSlotTable::find(int32_t kf_id) const {
  const auto it = index.find(kf_id);
  return it == index.end() ? -1 : it->second;
}

bool LoopSlotTable::db_add(int32_t kf_id) {
  const int s = find(kf_id);
  if (s < 0 || slots[s].member) return false;
  slots[s].member = true;
  slots[s].seq = next_seq++;
  n_members++;
  return true;
}

bool LoopSlotTable::db_erase(int32_t kf_id) {
  const int s = find(kf_id);
  if (s < 0) return false;
  if (slots[s].member) {
    slots[s].member = false;
    n_members--;
  }
  return true;
}

double loop_finish_score(double sum, int scoring) {
  if (scoring == 1) {
    if (sum >= 1) return 1.0;
    return 1.0 - std::sqrt(1.0 - sum);
  }
  return -sum / 2.0;
}

void LoopDetector::reset(int scoring) {
  scoring_ = scoring;
  groups_.clear();
  err_.clear();
}

bool LoopDetector::check_graph(const mmt_covis_graph& g, int32_t kf_id) {
  if (g.n_kf < 0 || !g.ordered_start || !g.conn_start || !g.bad) return fail("null graph arrays");
  if (kf_id < 0 || kf_id >= g.n_kf)
    return fail("keyframe " + std::to_string(kf_id) + " is outside the graph");
  return true;
}

// the CSR row of keyframe id, every entry checked against the graph's size
bool LoopDetector::list_of(const mmt_covis_graph& g, const int32_t* start, const int32_t* list,
                           int32_t id, const int32_t** b, const int32_t** e) {
  if (id < 0 || id >= g.n_kf)
    return fail("keyframe " + std::to_string(id) + " is outside the graph");
  const int32_t s0 = start[id], s1 = start[id + 1];
  if (s0 < 0 || s1 < s0) return fail("graph: row starts are not ascending");
  if (s1 > s0 && !list) return fail("null graph arrays");
  for (int32_t i = s0; i < s1; i++)
    if (list[i] < 0 || list[i] >= g.n_kf) return fail("graph: a listed keyframe is outside it");
  *b = list + s0;
  *e = list + s1;
  return true;
}

bool LoopDetector::candidates(const LoopSlotTable& T, const LoopScore* sc, int32_t kf_id,
                              float min_score, const mmt_covis_graph& g,
                              std::vector<int32_t>& out) {
  out.clear();
  if (!check_graph(g, kf_id)) return false;
  if (T.find(kf_id) < 0) return fail("keyframe " + std::to_string(kf_id) + " has no stored vector");
  const int ns = (int)T.slots.size();

  // spConnectedKeyFrames = pKF->GetConnectedKeyFrames()
  const int32_t *cb, *ce;
  if (!list_of(g, g.conn_start, g.conn, kf_id, &cb, &ce)) return false;
  std::vector<uint8_t> connected((size_t)g.n_kf, 0);
  for (const int32_t* p = cb; p != ce; ++p) connected[*p] = 1;

  // lKFsSharingWords, in the reference's order
  std::vector<int32_t> sharing;
  for (int s = 0; s < ns; s++) {
    const LoopSlot& L = T.slots[s];
    if (!L.member || sc[s].common <= 0) continue;
    if (L.kf_id < 0 || L.kf_id >= g.n_kf)
      return fail("database keyframe " + std::to_string(L.kf_id) + " is outside the graph");
    if (!connected[L.kf_id]) sharing.push_back(s);
  }
  std::sort(sharing.begin(), sharing.end(), [&](int32_t a, int32_t b) {
    if (sc[a].first != sc[b].first) return sc[a].first < sc[b].first;
    return T.slots[a].seq < T.slots[b].seq;
  });
  if (sharing.empty()) return true;

  std::vector<uint8_t> in_query((size_t)ns, 0);  // mnLoopQuery == pKF->mnId
  std::vector<float> loop_score((size_t)ns, 0.f);  // mLoopScore
  int maxCommonWords = 0;
  for (int32_t s : sharing) {
    in_query[s] = 1;
    if (sc[s].common > maxCommonWords) maxCommonWords = sc[s].common;
  }
  const int minCommonWords = (int)(maxCommonWords * 0.8f);

  std::vector<std::pair<float, int32_t>> lScoreAndMatch;
  for (int32_t s : sharing) {
    if (sc[s].common > minCommonWords) {
      const float si = (float)loop_finish_score(sc[s].sum, scoring_);
      loop_score[s] = si;
      if (si >= min_score) lScoreAndMatch.push_back(std::make_pair(si, s));
    }
  }
  if (lScoreAndMatch.empty()) return true;

  // accumulate score by covisibility
  std::vector<std::pair<float, int32_t>> lAccScoreAndMatch;
  float bestAccScore = min_score;
  for (const auto& it : lScoreAndMatch) {
    const int32_t s = it.second;
    const int32_t *nb, *ne;  // GetBestCovisibilityKeyFrames(10)
    if (!list_of(g, g.ordered_start, g.ordered, T.slots[s].kf_id, &nb, &ne)) return false;
    if (ne - nb > 10) ne = nb + 10;
    float bestScore = it.first;
    float accScore = it.first;
    int32_t best = s;
    for (const int32_t* p = nb; p != ne; ++p) {
      const int s2 = T.find(*p);
      if (s2 >= 0 && in_query[s2] && sc[s2].common > minCommonWords) {
        accScore += loop_score[s2];
        if (loop_score[s2] > bestScore) {
          best = s2;
          bestScore = loop_score[s2];
        }
      }
    }
    lAccScoreAndMatch.push_back(std::make_pair(accScore, best));
    if (accScore > bestAccScore) bestAccScore = accScore;
  }

  const float minScoreToRetain = 0.75f * bestAccScore;
  std::vector<uint8_t> added((size_t)ns, 0);  // spAlreadyAddedKF
  for (const auto& it : lAccScoreAndMatch) {
    if (it.first > minScoreToRetain && !added[it.second]) {
      out.push_back(T.slots[it.second].kf_id);
      added[it.second] = 1;
    }
  }
  return true;
}

bool LoopDetector::detect(LoopSlotTable& T, const LoopScore* sc, int32_t kf_id,
                          int32_t last_loop_kf_id, int consistency_th, const mmt_covis_graph& g,
                          int max_out, mmt_loop_result& res, std::vector<int32_t>& cand,
                          std::vector<int32_t>& enough) {
  cand.clear();
  enough.clear();
  res.ran = 0;
  res.min_score = 1.f;
  res.n_candidates = res.n_enough = 0;
  res.n_groups = (int32_t)groups_.size();
  const int slot = T.find(kf_id);
  if (slot < 0) return fail("keyframe " + std::to_string(kf_id) + " has no stored vector");
  if (T.slots[slot].member)
    return fail("keyframe " + std::to_string(kf_id) + " is in the database already");

  if (early_exit(kf_id, last_loop_kf_id)) {
    T.db_add(kf_id);
    return true;
  }
  if (!check_graph(g, kf_id)) return false;
  if (!sc) return fail("no scores");

  // the lowest score to a connected keyframe of the covisibility graph
  const int32_t *vb, *ve;  // GetVectorCovisibleKeyFrames
  if (!list_of(g, g.ordered_start, g.ordered, kf_id, &vb, &ve)) return false;
  float minScore = 1;
  for (const int32_t* p = vb; p != ve; ++p) {
    if (g.bad[*p]) continue;
    const int s = T.find(*p);
    if (s < 0)
      return fail("connected keyframe " + std::to_string(*p) + " has no stored vector");
    const float score = (float)loop_finish_score(sc[s].sum, scoring_);
    if (score < minScore) minScore = score;
  }

  if (!candidates(T, sc, kf_id, minScore, g, cand)) return false;
  if ((int64_t)cand.size() > (int64_t)max_out) return fail("output buffer too small");
  // a candidate's group is read before anything changes
  for (int32_t c : cand) {
    const int32_t *gb, *ge;
    if (!list_of(g, g.conn_start, g.conn, c, &gb, &ge)) return false;
  }
  res.ran = 1;
  res.min_score = minScore;
  res.n_candidates = (int32_t)cand.size();

  if (cand.empty()) {
    T.db_add(kf_id);
    groups_.clear();
    res.n_groups = 0;
    return true;
  }

  // consistency of each candidate's covisibility group with the previous groups
  std::vector<Group> vCurrentConsistentGroups;
  std::vector<bool> vbConsistentGroup(groups_.size(), false);
  for (size_t i = 0; i < cand.size(); i++) {
    const int32_t c = cand[i];
    const int32_t *gb, *ge;  // GetConnectedKeyFrames
    if (!list_of(g, g.conn_start, g.conn, c, &gb, &ge)) return false;
    std::vector<int32_t> group(gb, ge);
    group.push_back(c);
    std::sort(group.begin(), group.end());
    group.erase(std::unique(group.begin(), group.end()), group.end());

    bool bEnoughConsistent = false;
    bool bConsistentForSomeGroup = false;
    for (size_t iG = 0; iG < groups_.size(); iG++) {
      const std::vector<int32_t>& prev = groups_[iG].first;
      bool bConsistent = false;
      for (int32_t m : group) {
        if (std::binary_search(prev.begin(), prev.end(), m)) {
          bConsistent = true;
          bConsistentForSomeGroup = true;
          break;
        }
      }
      if (bConsistent) {
        const int nCurrentConsistency = groups_[iG].second + 1;
        if (!vbConsistentGroup[iG]) {
          vCurrentConsistentGroups.push_back(std::make_pair(group, nCurrentConsistency));
          vbConsistentGroup[iG] = true;
        }
        if (nCurrentConsistency >= consistency_th && !bEnoughConsistent) {
          enough.push_back(c);
          bEnoughConsistent = true;
        }
      }
    }
    if (!bConsistentForSomeGroup) vCurrentConsistentGroups.push_back(std::make_pair(group, 0));
  }
  groups_ = std::move(vCurrentConsistentGroups);
  T.db_add(kf_id);
  res.n_enough = (int32_t)enough.size();
  res.n_groups = (int32_t)groups_.size();
  return true;
}

}  // namespace mmt
