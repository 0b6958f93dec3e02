// multimot_track_amd/csrc/mmt_mapgraph.h -- the ORB-SLAM2 map graph: MapPoint and KeyFrame
// bookkeeping (observations, covisibility graph, spanning tree) and the local point list cache
// that reads it.  Host C++ without a device header: MapEngine (mmt_map.h) owns one of each, and
// tests/mapgraph_host_check.cpp drives them alone.
//
// Reference: MapPoint.cc, KeyFrame.cc, Map.cc; Tracking.cc:3555-3604 (expand_local_kfs),
// 3508-3534 (UpdateLocalPoints: LocalPointCache).
//
// The guard: everything UpdateLocalKeyFrames' expansion and UpdateLocalPoints read -- a stored
// keyframe's mps, ordered, parent, children and bad, a real point's bad -- is private to its
// record, readable through const getters and written by MapGraph's mutators only, each of which
// bumps the structure epoch.  A point list built at one epoch from an equal keyframe list is
// therefore the list a walk would build, which is what LocalPointCache relies on.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <map>
#include <memory>
#include <set>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/mmt.h"
#include "mmt_bowvec.h"

namespace mmt {

// An array in chunks of 2^kShift elements: indexing as a vector's (one more load), push_back never
// moves the elements already stored (references stay valid)
template <class T, int kShift = 13>
class ChunkArray {
 public:
  T& operator[](size_t i) { return chunks_[i >> kShift][i & kMask]; }
  const T& operator[](size_t i) const { return chunks_[i >> kShift][i & kMask]; }
  size_t size() const { return n_; }
  void push_back(const T& v) {
    if ((n_ >> kShift) >= chunks_.size()) chunks_.emplace_back(new T[kChunk]);
    (*this)[n_++] = v;
  }
  void clear() {
    chunks_.clear();
    n_ = 0;
  }

 private:
  static constexpr size_t kChunk = (size_t)1 << kShift, kMask = kChunk - 1;
  std::vector<std::unique_ptr<T[]>> chunks_;
  size_t n_ = 0;
};

class MapGraph;

// (the guarded fields sit where they always did: the record's layout is what the per-frame loops
// were measured with)
struct MPoint {
  float pos[3] = {0, 0, 0};
  float normal[3] = {0, 0, 0};
  float minDist = 0, maxDist = 0;
  uint8_t desc[32] = {0};

 private:
  friend class MapGraph;
  std::vector<std::pair<int, int>> obs_;  // mObservations (keyframe id, key index), id-ascending
  int nObs_ = 0;
  int refKF_ = -1;

 public:
  int firstKFid = -1;
  int visible = 1, found = 1;

 private:
  bool bad_ = false;

 public:
  bool trackInView = false;
  bool dirty = false;  // pool record out of date
  long lastSeen = 0;  // real points: mirrored in MapGraph's PtHot (the per-frame scans read that)

 private:
  int replaced_ = -1;  // mpReplaced

 public:
  long fuseCand = 0, baLocal = 0;  // mnFuseCandidateForKF, mnBALocalForKF
  int desc_ver = 0;   // bumped by ComputeDistinctiveDescriptors (Fuse results read it)
  const std::vector<std::pair<int, int>>& obs() const { return obs_; }
  int nObs() const { return nObs_; }
  int refKF() const { return refKF_; }
  bool bad() const { return bad_; }
  int replaced() const { return replaced_; }
  int obs_index(int kf) const {
    for (const auto& o : obs_)
      if (o.first == kf) return o.second;
    return -1;
  }
};

struct KFrame {
  int id = 0;
  long frameId = 0;
  float Tcw[16], Twc[16], Ow[3];  // written by MapGraph::set_pose
  std::vector<mmt_kp> keys;
  std::vector<float> uR, depth;
  std::vector<uint8_t> desc;
  long trackRef = 0;
  long fuseTarget = 0, baLocal = 0, baFixed = 0;  // mnFuseTargetForKF, mnBALocalForKF, mnBAFixedForKF
  // with a vocabulary: mBowVec, mFeatVec, and the KeyFrameDatabase query fields (KeyFrame.h:146-149;
  // mRelocScore uninitialised in the reference: pinned 0)
  BowVecH bow;
  FeatVecH fv;
  bool hasBow = false;
  long relocQuery = 0;
  int relocWords = 0;
  float relocScore = 0;
  const std::vector<int>& mps() const { return mps_; }
  const std::map<int, int>& conn() const { return conn_; }  // mConnectedKeyFrameWeights
  const std::vector<int>& ordered() const { return ordered_; }
  int parent() const { return parent_; }
  const std::set<int>& children() const { return children_; }
  bool bad() const { return bad_; }

 private:
  friend class MapGraph;
  std::vector<int> mps_;
  std::map<int, int> conn_;
  std::vector<int> ordered_;
  bool firstConnection_ = true;
  int parent_ = -1;
  std::set<int> children_;
  bool bad_ = false;
};

// the fields the per-frame local-map scans read, one compact record per real point (point index):
// UpdateLocalPoints walks ~13k point references and SearchLocalPoints ~4.4k, at random, and a
// 12-byte record keeps them in cache where the 136-byte MPoint does not
struct PtHot {
  int trackRef = 0;  // mnTrackReferenceForFrame
  int lastSeen = 0;  // mnLastFrameSeen
  bool bad() const { return bad_ != 0; }

 private:
  friend class MapGraph;
  uint8_t bad_ = 0;
};
static_assert(sizeof(PtHot) == 12, "PtHot outgrew its 12 bytes");

// The map-path view of one Frame: its ORB output and B3 arrays (host copies of the device ones)
// and its map state.
struct MapFrameH {
  long id = 0;
  int n = 0;
  const mmt_kp* kps = nullptr;
  const uint8_t* desc = nullptr;
  const float* uR = nullptr;     // mvuRight
  const float* depth = nullptr;  // mvDepth
  std::vector<int> mps;          // mvpMapPoints (point handle or -1)
  std::vector<uint8_t> outlier;  // mvbOutlier
  int refKF = -1;                // mpReferenceKF
  BowVecH bow;                   // mBowVec / mFeatVec (Frame::ComputeBoW, with a vocabulary)
  FeatVecH fv;
  bool hasBow = false;
};

class MapGraph {
 public:
  // handles from kTemp up are Tracking's temporary (VO) points: never in a keyframe, never in the
  // local map, so their edits need no epoch
  static constexpr int kTemp = 1 << 29;
  // scale: mvScaleFactors of the nlevels pyramid levels (UpdateNormalAndDepth); profile: time
  // compute_distinctive (stats().distinctive_us)
  void setup(const std::vector<float>& scale, int nlevels, bool profile);
  void reset();  // Map::clear; KeyFrame::nNextId = 0

  // ---- reads
  long epoch() const { return struct_epoch_; }
  size_t n_kfs() const { return kfs_.size(); }  // stored keyframes, bad ones included
  int n_keyframes() const;                      // Map::KeyFramesInMap
  int n_mappoints() const { return n_good_; }   // non-bad map points
  size_t n_points() const { return pts_.size(); }  // real points allocated (handles below it)
  const KFrame& kf(int k) const { return kfs_[k]; }
  KFrame& kf(int k) { return kfs_[k]; }  // the unguarded fields are the caller's to write
  const MPoint& mp(int h) const { return h >= kTemp ? temps_[h - kTemp] : pts_[h]; }
  MPoint& mp(int h) { return h >= kTemp ? temps_[h - kTemp] : pts_[h]; }
  const PtHot& hot(int h) const { return hot_[h]; }  // real points only
  PtHot& hot(int h) { return hot_[h]; }
  // host prefetch of map point h's record (loops over point lists walk a 100k-point map in
  // random order: one cache miss per record otherwise); MMT_NO_PREFETCH builds without it (A/B)
  void prefetch_point(int h) const {
#ifndef MMT_NO_PREFETCH
    if (h >= 0 && h < kTemp && (size_t)h < pts_.size()) __builtin_prefetch(&pts_[h]);
#else
    (void)h;
#endif
  }
  int tracked_map_points(int kf, int minObs) const;  // KeyFrame::TrackedMapPoints
  // the map as flat arrays (mmt_map_dump, include/mmt.h): sizes[7]; arrays written when out != 0
  void dump(int32_t* sizes, const mmt_map_dump_arrays* out) const;
  // UpdateLocalKeyFrames' second part (Tracking.cc:3555-3604): per keyframe of the counted set, its
  // first unmarked good covisible among the best 10, its first unmarked good child, and its parent
  // (which ends the loop), up to 80 keyframes
  template <class Marked, class Mark>
  void expand_local_kfs(std::vector<int>& kfl, Marked marked, Mark mark) const;

  // ---- MapPoint edits
  int new_point_kf(const float* pos, int kf);  // MapPoint(Pos, pRefKF, pMap)
  int new_temp_point(const MPoint& p);         // MapPoint(Pos, pMap, pFrame, idxF): a handle >= kTemp
  void reserve_temps(size_t n) { temps_.reserve(n); }
  void clear_temps() { temps_.clear(); }
  void add_observation(int h, int kf, int idx);
  void erase_observation(int h, int kf);
  void set_bad(int h);
  void replace(int h, int by);
  void compute_distinctive(int h);
  void update_normal_depth(int h);
  // the device pool's record of point h is out of date: the points so marked, in marking order,
  // until dirty_flushed() (whose caller has cleared each one's MPoint::dirty)
  void mark_dirty(int h);
  const std::vector<int>& dirty() const { return dirty_; }
  void dirty_flushed() { dirty_.clear(); }

  // ---- KeyFrame edits
  int new_keyframe(const MapFrameH& C, const float* Tcw);  // KeyFrame(F, ...)
  void set_pose(int kf, const float* Tcw);
  void kf_set_mp(int kf, int idx, int h);  // AddMapPoint / EraseMapPointMatch / ReplaceMapPointMatch
  void add_connection(int kf, int other, int w);
  void erase_connection(int kf, int other);
  void update_connections(int kf);
  void kf_set_bad(int kf);  // KeyFrame::SetBadFlag but for the database's erase (the caller's)

  struct Stats {
    long n_reparent = 0;        // spanning-tree children re-parented by kf_set_bad
    double distinctive_us = 0;  // host wall time inside compute_distinctive (setup's profile)
  };
  const Stats& stats() const { return stats_; }

 private:
  void mark_bad(int h);  // mbBad, the map's point count, the per-frame scan record
  void update_best_covisibles(int kf);
  // bumped by every edit of what expand_local_kfs and LocalPointCache's walk read (see the top)
  long struct_epoch_ = 0;
  // map points in fixed chunks: growing the array never moves the existing points (a vector's
  // reallocation moved all of them, 100k points at a time, inside a keyframe's point creation)
#ifdef MMT_PTS_VECTOR  // A/B build (tools/build_prof_lib.sh)
  std::vector<MPoint> pts_;
#else
  ChunkArray<MPoint> pts_;
#endif
  std::vector<MPoint> temps_;
  std::vector<PtHot> hot_;
  std::vector<KFrame> kfs_;
  int kfNextId_ = 0;
  int n_good_ = 0;
  std::vector<int> dirty_;
  // compute_distinctive's pairwise descriptor distances of points with more than 32 good
  // observations, by observation ((keyframe << 32) | key, keyframe order)
  struct DistCache {
    std::vector<uint64_t> ids;
    std::vector<uint16_t> d;
  };
  std::unordered_map<int, DistCache> dcache_;
  std::vector<float> scale_;
  int nlevels_ = 0;
  bool prof_on_ = false;
  Stats stats_;
};

template <class Marked, class Mark>
void MapGraph::expand_local_kfs(std::vector<int>& kfl, Marked marked, Mark mark) const {
  const size_t n0 = kfl.size();
  for (size_t q = 0; q < n0; q++) {
    if (kfl.size() > 80) break;
    const KFrame& K = kfs_[kfl[q]];
    const size_t nn = std::min<size_t>(10, K.ordered_.size());
    for (size_t a = 0; a < nn; a++) {
      const int id = K.ordered_[a];
      if (!kfs_[id].bad_ && !marked(id)) {
        kfl.push_back(id);
        mark(id);
        break;
      }
    }
    for (int ch : K.children_) {
      if (!kfs_[ch].bad_ && !marked(ch)) {
        kfl.push_back(ch);
        mark(ch);
        break;
      }
    }
    if (K.parent_ >= 0 && !marked(K.parent_)) {
      kfl.push_back(K.parent_);
      mark(K.parent_);
      break;  // leaves the keyframe loop (Tracking.cc:3601)
    }
  }
}

// Tracking::UpdateLocalPoints over a keyframe list, with the walk's result kept.  Between two
// keyframes nothing the walk reads changes, and with the dense covisibility of the vocabulary
// path the keyframe list is the frame before's too: the list of a walk is handed out again while
// the keyframe list and the graph's epoch stay as they were when it was built.  The graph comes
// in by const reference: the cache cannot edit what it caches.
// mode (MMT_LOCALMAP_CACHE): 1 a call with an equal keyframe list at an unchanged epoch takes the
// cached points; 0 walks every time (A/B); 2 also walks on every hit and reports a difference.
// ways (MMT_LOCALMAP_CACHE_WAYS, 1-8): that many lists of the current epoch are kept, the least
// recently used one replaced (the counted keyframe set flickers at its margin from frame to frame
// and comes back: §5h of DESIGN.md).
class LocalPointCache {
 public:
  static constexpr int kMaxWays = 8;
  explicit LocalPointCache(int mode = 1, int ways = 4);
  // out: the local points of the keyframes kfl; gen: the generation of the list out holds, in
  // and out (a list with an equal generation is equal element for element).  False: mode 2 found
  // the cached list different from the walk's (check() holds the walk's).
  bool collect(const MapGraph& g, const std::vector<int>& kfl, std::vector<int>& out, long& gen);
  void walk(const MapGraph& g, const std::vector<int>& kfl, std::vector<int>& out);
  long new_gen() { return ++list_gen_; }  // for a list the caller builds itself
  int mode() const { return mode_; }
  long hits() const { return hits_; }
  long rebuilds() const { return rebuilds_; }
  long epoch_rebuilds() const { return new_epoch_; }  // the rebuilds after a structure edit
  const std::vector<int>& check() const { return check_; }

 private:
  int mode_, ways_;
  // The keyframe list and point list of the last walks (copies: the caller swaps the vectors it
  // holds), each list's generation and the epoch they were built at (one for all: a structure
  // edit drops every kept list)
  struct Entry {
    std::vector<int> kfs, pts;
    long gen = 0, used = 0;
    bool valid = false;
  };
  Entry e_[kMaxWays];
  std::vector<int> check_;
  long epoch_ = -1, tick_ = 0, hits_ = 0, rebuilds_ = 0, new_epoch_ = 0;
  long list_gen_ = 0;              // the last generation handed out
  std::vector<int> buf_;           // walk's compacted slots
  std::vector<uint64_t> seen_;     // walk's per-point marks (bits)
};

}  // namespace mmt
