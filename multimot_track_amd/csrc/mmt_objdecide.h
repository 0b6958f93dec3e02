// multimot_track_amd/csrc/mmt_objdecide.h -- the host half of the object front end: which
// semantic labels of a frame become objects (B7 decisions, Tracking.cc:1424-1536) and which motion
// label each one carries on from the last frame (B8, Tracking.cc:1556-1630), over the per-label
// statistics and the current x last label histogram k_obj_group (mmt_track.hip) writes.
// Plain C++, no device headers: tests/objdecide_host_check.cpp builds it alone.
#pragma once
#include <vector>

namespace mmt {

constexpr int kMaxLabel = 16;  // semantic labels 0..15 per frame (LoadMask keeps 1..3)

// k_obj_group's record for one semantic label (32 bytes, read back as written)
struct LabelStats {
  int cnt, bcnt, sfcnt, members;
  float depth_sum;
  int pad[3];
};

struct ObjDecision {
  std::vector<int> labels;  // SemPosNew: semantic label of each kept object, ascending
  std::vector<int> LabId;   // nModLabel: motion label of each kept object
};

// stats[kMaxLabel], hist[kMaxLabel][kMaxLabel] (current label x last label member counts);
// bSecond: the frame after the first one; lastModLabel / lastSemPosition: the last frame's
// nModLabel / nSemPosition (same length).
//
// A label is kept unless more than half of its samples lie in the boundary band, it has at most
// 100 samples, more than 0.3 of them have a scene flow under the threshold, or their mean depth
// exceeds 25 (ratios in float, as the reference's float counters divided by a size_t are).  A
// kept object takes the motion label of the last-frame object whose semantic label most of its
// samples had in the last frame (the smallest such label on equal counts: std::sort of at most 15
// pairs is an insertion sort, which keeps std::map's ascending order), or a fresh one.  The first
// fresh label is max(lastModLabel) + 1; the reference leaves it uninitialised when the last frame
// had no object (Tracking.cc:1557-1568) -- pinned 1 here.
ObjDecision obj_decide(const LabelStats* stats, const int* hist, bool bSecond,
                       const std::vector<int>& lastModLabel,
                       const std::vector<int>& lastSemPosition);

}  // namespace mmt
