// multimot_track_amd/csrc/mmt_map.hip -- ORB-SLAM2 map tracking for RGB-D (see mmt_map.h).
//
// cv::Mat float arithmetic as elsewhere on the host side of this path: products accumulate in
// double and round to float, the translation is added in float; Mat / scalar is * (1.0 / s) in
// double; cv::norm is the double square root of the double sum of squares.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>

#include "mmt_map.h"
#include "mmt_mat4.h"

namespace mmt {

#define MAP_PROF(k, stmt)                       \
  do {                                          \
    const double _t0 = prof_on_ ? now_us() : 0; \
    stmt;                                       \
    if (prof_on_) prof_[k] += now_us() - _t0;   \
  } while (0)

MapEngine::~MapEngine() {
  if (prof_on_ && prof_n_ > 0) {
    static const char* names[12] = {"C2 search", "D1 (motion model)", "local map update",
                                    "C3 search", "D1 (local map)", "keyframe + mapping",
                                    "other", "total", "UpdateLastFrame", "C2 pack",
                                    "C3 pack", "D1 pack"};
    fprintf(stderr, "[mmt map profile] %ld frames, host wall us per frame:", prof_n_);
    for (int k = 0; k < 12; k++) fprintf(stderr, " %s %.1f%s", names[k], prof_[k] / prof_n_,
                                         k < 11 ? "," : "\n");
    if (mstats_.n_lm > 0) {
      const double n = (double)mstats_.n_lm;
      fprintf(stderr, "[mmt localmapping profile] %ld keyframes, host wall us per keyframe: "
              "ProcessNewKeyFrame+MapPointCulling %.1f, CreateNewMapPoints + SearchInNeighbors %.1f "
              "(CreateNewMapPoints %.1f, Fuse launches "
              "%.1f), LocalBundleAdjustment %.1f (solve %.1f), KeyFrameCulling %.1f, final sync "
              "%.1f, LocalMapping total %.1f; CreateNewKeyFrame with all of it %.1f\n", mstats_.n_lm,
              mstats_.pnk_us / n,
              mstats_.sin_us / n, mstats_.cnmp_us / n, mstats_.fuse_us / n, mstats_.ba_us / n,
              mstats_.basolve_us / n, mstats_.cull_us / n, mstats_.lmsync_us / n,
              mstats_.lm_us / n, mstats_.kfnew_us / n);
      static const char* bn[MappingStats::kBlk] = {
          "new keyframe + store", "new points", "SIN targets", "SIN fuse 1", "SIN candidates",
          "SIN fuse 2", "SIN point updates", "SIN connections", "BA graph", "BA apply",
          "Fuse pool flush", "Fuse enqueue", "Fuse wait", "Fuse apply (+ relaunches)",
          "ComputeDistinctiveDescriptors (inside the others)", "PNK ComputeBoW",
          "PNK observations", "PNK UpdateConnections"};
      fprintf(stderr, "[mmt localmapping profile] per keyframe, us:");
      for (int k = 0; k < MappingStats::kBlk; k++)
        fprintf(stderr, " %s %.1f%s", bn[k],
                (k == 14 ? graph_.stats().distinctive_us : mstats_.blk_us[k]) / n,
                k + 1 < MappingStats::kBlk ? "," : "\n");
    }
    fprintf(stderr, "[mmt map profile] per frame: %.1f local keyframes, %.1f local points, "
            "%.1f C3 edges; %zu map points allocated, %d keyframes at the end; local map "
            "speculated %ld times, taken %ld; local point list cache (MMT_LOCALMAP_CACHE=%d) "
            "hits %ld, rebuilds %ld (%ld of them after a structure edit, %ld ids uploads); flow "
            "solves (MMT_D2_CHAIN=%d) chained %ld, host-launched %ld, redone %ld\n",
            prof_cnt_[0] / prof_n_, prof_cnt_[1] / prof_n_, prof_cnt_[2] / prof_n_, graph_.n_points(),
            n_keyframes(), spec_tries_, spec_hits_, lpc_.mode(), lpc_.hits(), lpc_.rebuilds(),
            lpc_.epoch_rebuilds(), ids_uploads_, d2_chain_mode_, d2_count_[0], d2_count_[1],
            d2_count_[2]);
  }
  if (s_) (void)hipStreamSynchronize(s_);
  if (lm_s_) {
    (void)hipStreamSynchronize(lm_s_);
    (void)hipStreamDestroy(lm_s_);
  }
  if (ev_early_) (void)hipEventDestroy(ev_early_);
  if (ev_d1_) (void)hipEventDestroy(ev_d1_);
  for (void* p : dallocs_) (void)hipFree(p);
  for (void* p : hallocs_) (void)hipHostFree(p);
}

static size_t last_bytes(int n) { return (size_t)n * (sizeof(mmt_kp) + 12 + 32 + 2); }

// every chain (C2 -> D1, C3 -> D1) moves one block up and one block down
static_assert(sizeof(PoseOptDesc) <= kDescBytes, "PoseOptDesc outgrew its slot");
static size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// C3's upload block for m local points and n keys: offsets of taken (after ids, skip), the base
// positions and their flags, and the total size
// (ids_inline false: the ids have a buffer of their own and no room here)
struct SelLayout {
  size_t ids, skip, taken, bX, bHas, total;
  SelLayout(int m, int n, bool ids_inline = true) {
    ids = kDescBytes;
    skip = ids + (ids_inline ? 4 * (size_t)m : 0);
    taken = skip + m;
    bX = align16(taken + n);
    bHas = bX + 12 * (size_t)n;
    total = bHas + n;
  }
};

size_t MapEngine::out_bytes(int n) const { return kOutHdr + 4 * (size_t)kcap_ + n; }

void MapEngine::setup(const MapCamH& cam, int kcap) {
  cam_ = cam;
  kcap_ = kcap;
  d_last_ = dev<uint8_t>(kDescBytes + last_bytes(kcap));
  h_last_ = pinned<uint8_t>(kDescBytes + last_bytes(kcap));
  c2_ = CandSet{dev<uint32_t>((size_t)kcap * kCandK), dev<int>((size_t)kcap * kCandK),
                dev<int>(kcap), dev<PointWin>(kcap), dev<int>(kcap)};
  d_out_ = dev<uint8_t>(kOutHdr + 5 * (size_t)kcap);
  h_out_ = pinned<uint8_t>(kOutHdr + 5 * (size_t)kcap);
  d_nm_ = (int*)d_out_;
  d_ninl_ = (int*)(d_out_ + 4);
  d_pose_ = (float*)(d_out_ + 16);
  d_match_ = (int*)(d_out_ + kOutHdr);
  d_outl_ = d_out_ + kOutHdr + 4 * (size_t)kcap;
  h_nm_ = (int*)h_out_;
  h_ninl_ = (int*)(h_out_ + 4);
  h_pose_ = (float*)(h_out_ + 16);
  h_match_ = (int*)(h_out_ + kOutHdr);
  h_outl_ = h_out_ + kOutHdr + 4 * (size_t)kcap;
  d_edges_ = dev<float>(7 * (size_t)kcap);
  h_edges_ = pinned<float>(7 * (size_t)kcap);
  d_esc_ = dev<double>(3 * (size_t)kcap);
  d_fsc_ = dev<int>(kcap);
  prof_on_ = getenv("MMT_MAP_PROFILE") != nullptr;
  if (const char* e = getenv("MMT_LOCALMAP_SPEC")) spec_on_ = atoi(e) != 0;
  if (const char* e = getenv("MMT_OVERLAP_C3")) overlap_c3_ = atoi(e) != 0;
  int lpc_mode = 1, lpc_ways = 4;
  if (const char* e = getenv("MMT_LOCALMAP_CACHE")) lpc_mode = atoi(e);
  if (const char* e = getenv("MMT_LOCALMAP_CACHE_WAYS")) lpc_ways = atoi(e);
  lpc_ = LocalPointCache(lpc_mode, lpc_ways);
  graph_.setup(cam_.scale, cam_.nlevels, prof_on_);
  h_early_ = pinned<uint8_t>(kOutHdr + 4 * (size_t)kcap);
  MMT_HIP(hipEventCreateWithFlags(&ev_early_, hipEventDisableTiming));
  MMT_HIP(hipEventCreateWithFlags(&ev_d1_, hipEventDisableTiming));
  // LocalMapping's stream, normal priority (high / low measured within noise / slower in round 5,
  // without the vocabulary): its kernels (keyframe store copies, the BoW transform, Fuse,
  // SearchForTriangulation, the local BA) need nothing of the frame's flow solve.  MMT_LM_PRIO=high
  // (A/B): the greatest priority
  int prio_lo = 0, prio_hi = 0;
  MMT_HIP(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
  const char* lmp = getenv("MMT_LM_PRIO");
  const int lm_prio = lmp && strcmp(lmp, "high") == 0 ? prio_hi : 0;
  MMT_HIP(hipStreamCreateWithPriority(&lm_s_, hipStreamNonBlocking, lm_prio));
  // keyframe store record: keys, descriptors, mvuRight, grid (cell starts + key lists)
  kf_rec_bytes_ = align16(sizeof(mmt_kp) * (size_t)kcap) + 32 * (size_t)kcap +
                  align16(4 * (size_t)kcap) + align16(4 * (size_t)(kGridCells + 1)) +
                  align16(4 * (size_t)kcap);
  frameNextId_ = 0;
  mbVO_ = false;
  matchesInliers_ = 0;
  lastRelocFrameId_ = 0;
  reset();
}

// the local-map buffers grow with the local map; the point pool with the map
void MapEngine::grow_local(int m) {
  if (m <= local_cap_ && d_sel_) return;
  const int cap = std::max(m + 4096, 2 * local_cap_);
  void* old[] = {d_sel_, h_sel_, d_inview_, h_inview_, c3_.key, c3_.idx, c3_.n, c3_.win,
                 c3_.choice, d_ids_, h_ids_};
  if (s_) MMT_HIP(hipStreamSynchronize(s_));
  for (int i = 0; i < 11; i++) {
    if (!old[i]) continue;
    const bool host = i == 1 || i == 3 || i == 10;
    auto it = std::find(host ? hallocs_.begin() : dallocs_.begin(),
                        host ? hallocs_.end() : dallocs_.end(), old[i]);
    if (host) {
      (void)hipHostFree(old[i]);
      hallocs_.erase(it);
    } else {
      (void)hipFree(old[i]);
      dallocs_.erase(it);
    }
  }
  const size_t sel_cap = SelLayout(cap, kcap_).total + 16;
  d_sel_ = dev<uint8_t>(sel_cap);
  h_sel_ = pinned<uint8_t>(sel_cap);
  d_inview_ = dev<uint8_t>(cap);
  h_inview_ = pinned<uint8_t>(cap);
  c3_ = CandSet{dev<uint32_t>((size_t)cap * kCandK), dev<int>((size_t)cap * kCandK), dev<int>(cap),
                dev<PointWin>(cap), dev<int>(cap)};
  d_ids_ = dev<int>(cap);
  h_ids_ = pinned<int>(cap);
  ids_gen_ = -1;  // the new buffer holds no list
  local_cap_ = cap;
}

void MapEngine::reset() {
  graph_.reset();
  kf_dev_.clear();
  spec_discard();
  state_ = 0;
  frameNextId_ = 0;  // Frame::nNextId = 0 (Tracking.cc:3808)
  lastKFFrameId_ = 0;
  refKF_ = -1;
  localKFs_.clear();
  localPts_.clear();
  local_gen_ = lpc_.new_gen();
  recent_.clear();
  hasTlr_ = false;
  snapKF_ = -1;
  for (auto& l : invfile_) l.clear();  // mpKeyFrameDB->clear() (Tracking.cc:3801)
}

void MapEngine::prepare(MapFrameH& F) const {
  F.mps.assign(F.n, -1);
  F.outlier.assign(F.n, 0);
  F.refKF = -1;
  F.hasBow = false;
  F.bow.word.clear();
  F.bow.value.clear();
  F.fv = FeatVecH();
}

void MapEngine::process_new_keyframe(int kf) {  // LocalMapping::ProcessNewKeyFrame
  double tb = prof_on_ ? now_us() : 0;
  // mpCurrentKeyFrame->ComputeBoW() (without a vocabulary: none): the descent runs on the GPU
  // while the observations and connections below are updated on the host (they do not read it)
  if (voc_) kf_bow_launch(kf);
  blk_time(15, tb);
  const std::vector<int> mps = graph_.kf(kf).mps();
  for (size_t i = 0; i < mps.size(); i++) {
    const int h = mps[i];
    if (h < 0 || graph_.mp(h).bad()) continue;
    if (graph_.mp(h).obs_index(kf) < 0) {
      graph_.add_observation(h, kf, (int)i);
      graph_.update_normal_depth(h);
      graph_.compute_distinctive(h);
    } else {
      recent_.push_back(h);
    }
  }
  blk_time(16, tb);
  graph_.update_connections(kf);
  blk_time(17, tb);
  if (voc_) kf_bow_finish(kf);
  blk_time(15, tb);
}

void MapEngine::map_point_culling(int kf) {  // LocalMapping::MapPointCulling (RGB-D: 3 obs)
  const int cur = graph_.kf(kf).id;
  std::vector<int> keep;
  keep.reserve(recent_.size());
  for (int h : recent_) {
    MPoint& p = graph_.mp(h);
    if (p.bad()) continue;
    if ((float)p.found / p.visible < 0.25f) {
      graph_.set_bad(h);
    } else if (cur - p.firstKFid >= 2 && p.nObs() <= 3) {
      graph_.set_bad(h);
    } else if (cur - p.firstKFid < 3) {
      keep.push_back(h);
    }
  }
  recent_.swap(keep);
}

// ------------------------------------------------------------------ GPU stages
// D1's descriptor for an edge list that k_match_fix builds on the device (it writes n): the edge
// arrays at a fixed capacity of kcap edges
void MapEngine::pose_desc_fill(uint8_t* h_blk, uint8_t* d_blk, const float* Tcw) {
  h_pod_ = (PoseOptDesc*)h_blk;
  d_pod_ = (PoseOptDesc*)d_blk;
  PoseOptDesc& d = *h_pod_;
  memset(&d, 0, sizeof(d));
  d.n = 0;
  d.Xw = d_edges_;
  d.obs = d_edges_ + 3 * (size_t)kcap_;
  d.inv_sigma2 = d_edges_ + 6 * (size_t)kcap_;
  memcpy(d.Tcw, Tcw, 64);
  d.fx = cam_.fx; d.fy = cam_.fy; d.cx = cam_.cx; d.cy = cam_.cy; d.bf = cam_.bf;
  d.pose_out = d_pose_;
  d.outlier = d_outl_;
  d.n_inliers = d_ninl_;
  d.e_scratch = d_esc_;
  d.f_scratch = d_fsc_;
}

MapEdgeArgs MapEngine::edge_args(const GridFrame& G) const {
  MapEdgeArgs e;
  memset(&e, 0, sizeof(e));
  e.n = G.n;
  e.keys = G.keys;
  e.uR = G.uR;
  e.match = d_match_;
  for (int l = 0; l < cam_.nlevels && l < kMaxLevels; l++) e.inv_sigma2[l] = cam_.invSigma2[l];
  e.X = d_edges_;
  e.obs = d_edges_ + 3 * (size_t)kcap_;
  e.s2 = d_edges_ + 6 * (size_t)kcap_;
  e.desc = d_pod_;
  return e;
}

// Optimizer::PoseOptimization's results for the frame's MapPoints (edges in key order): every
// edge's mvbOutlier is reset, and below 3 edges the pose stays (Optimizer.cc:3160-3253)
void MapEngine::apply_pose_opt(MapFrameH& C, float* Tcw) {
  int n = 0;
  for (int i = 0; i < C.n; i++)
    if (C.mps[i] >= 0) {
      C.outlier[i] = 0;
      n++;
    }
  if (n < 3) return;
  memcpy(Tcw, h_pose_, 64);
  int e = 0;
  for (int i = 0; i < C.n; i++)
    if (C.mps[i] >= 0) C.outlier[i] = h_outl_[e++];
}

// SearchByProjection(CurrentFrame, LastFrame, th, bMono=false) with mbCheckOrientation, retried at
// retry_th while it finds fewer than min_matches (retry_th 0: no retry), then PoseOptimization on
// its matches when there are at least min_matches -- the whole chain on the device, one sync.
// Returns nmatches; the pose and outliers are applied when D1 ran.
int MapEngine::gpu_frame_chain(MapFrameH& C, const GridFrame& G, float* Tcw, const MapFrameH& L,
                               const float* Tlast, float th, float retry_th, int min_matches,
                               int retry_below, bool spec) {
  if (retry_below < 0) retry_below = min_matches;
  const double t_pack = prof_on_ ? now_us() : 0;
  const int n1 = L.n;
  uint8_t* hk = h_last_ + kDescBytes;
  float* hX = (float*)(hk + (size_t)n1 * sizeof(mmt_kp));
  uint8_t* hD = (uint8_t*)(hX + 3 * (size_t)n1);
  uint8_t* hA = hD + 32 * (size_t)n1;
  uint8_t* hO = hA + n1;
  memcpy(hk, L.kps, sizeof(mmt_kp) * (size_t)n1);
  int nact = 0;
  for (int i = 0; i < n1; i++) {
    const int h = L.mps[i];
    hA[i] = h >= 0 && !L.outlier[i];
    nact += hA[i];
    hO[i] = 0;
    if (h >= 0) {
      const MPoint& p = graph_.mp(h);
      memcpy(hX + 3 * (size_t)i, p.pos, 12);
      memcpy(hD + 32 * (size_t)i, p.desc, 32);
      hO[i] = p.nObs() > 0;
    }
  }
  if (prof_on_) prof_[9] += now_us() - t_pack;
  pose_desc_fill(h_last_, d_last_, Tcw);
  MMT_HIP(hipMemcpyAsync(d_last_, h_last_, kDescBytes + last_bytes(n1), hipMemcpyHostToDevice,
                         s_));
  LastFrameDev LD;
  LD.keys = (const mmt_kp*)(d_last_ + kDescBytes);
  LD.Xw = (const float*)(d_last_ + kDescBytes + (size_t)n1 * sizeof(mmt_kp));
  LD.mp_desc = (const uint8_t*)(LD.Xw + 3 * (size_t)n1);
  LD.active = LD.mp_desc + 32 * (size_t)n1;
  LD.obs = LD.active + n1;
  LD.n = n1;
  memcpy(LD.Tcw, Tlast, 64);
  // D1's edges are built by the matcher kernels from their final bindings
  MapEdgeArgs e = edge_args(G);
  e.nm = d_nm_;
  e.min_matches = min_matches;
  e.src_X = LD.Xw;
  launch_sbp_frame(G, Tcw, LD, th, 0, 1, c2_, d_match_, d_nm_, s_, nullptr, 0, &e);
  if (retry_th > 0)
    launch_sbp_frame(G, Tcw, LD, retry_th, 0, 1, c2_, d_match_, d_nm_, s_, d_nm_, retry_below, &e);
  spec = spec && spec_on_;
  if (spec) {  // the final matches (D1 does not change them) ahead of D1, for speculate_local_map
    MMT_HIP(hipMemcpyAsync(h_early_, d_out_, kOutHdr + 4 * (size_t)C.n, hipMemcpyDeviceToHost, s_));
    MMT_HIP(hipEventRecord(ev_early_, s_));
  }
  launch_pose_opt(d_pod_, 1, std::min(C.n, nact), s_);
  MMT_HIP(hipMemcpyAsync(h_out_, d_out_, out_bytes(C.n), hipMemcpyDeviceToHost, s_));
  if (!spec || !overlap_c3_) run_overlap();
  if (spec) {
    MMT_HIP(hipEventSynchronize(ev_early_));
    if (*(const int*)h_early_ >= min_matches) speculate_local_map(L, C.n);
  }
  MMT_HIP(hipStreamSynchronize(s_));
  std::fill(C.mps.begin(), C.mps.end(), -1);
  for (int i2 = 0; i2 < C.n; i2++)
    if (h_match_[i2] >= 0) C.mps[i2] = L.mps[h_match_[i2]];
  const int nm = *h_nm_;
  if (nm >= min_matches) apply_pose_opt(C, Tcw);
  return nm;
}

void MapEngine::gpu_flush_pool(hipStream_t st) {
  if (!st) st = s_;
  // grow the pool with the map, then scatter the changed records
  if ((int)graph_.n_points() > pool_cap_) {
    const int cap = std::max((int)graph_.n_points() + 8192, 2 * pool_cap_);
    LocalPointDev* np = nullptr;
    uint8_t* nd = nullptr;
    MMT_HIP(hipMalloc((void**)&np, sizeof(LocalPointDev) * (size_t)cap));
    MMT_HIP(hipMalloc((void**)&nd, 32 * (size_t)cap));
    if (pool_cap_ > 0) {
      MMT_HIP(hipMemcpyAsync(np, d_pool_, sizeof(LocalPointDev) * (size_t)pool_cap_,
                             hipMemcpyDeviceToDevice, st));
      MMT_HIP(hipMemcpyAsync(nd, d_pool_desc_, 32 * (size_t)pool_cap_, hipMemcpyDeviceToDevice,
                             st));
      MMT_HIP(hipStreamSynchronize(st));
      auto drop = [&](void* p) {
        dallocs_.erase(std::find(dallocs_.begin(), dallocs_.end(), p));
        (void)hipFree(p);
      };
      drop(d_pool_);
      drop(d_pool_desc_);
    }
    d_pool_ = np;
    d_pool_desc_ = nd;
    dallocs_.push_back(np);
    dallocs_.push_back(nd);
    pool_cap_ = cap;
  }
  const std::vector<int>& dirty = graph_.dirty();
  const int nd = (int)dirty.size();
  if (nd == 0) return;
  if (nd > up_cap_) {
    MMT_HIP(hipStreamSynchronize(st));
    if (d_up_) {
      dallocs_.erase(std::find(dallocs_.begin(), dallocs_.end(), (void*)d_up_));
      hallocs_.erase(std::find(hallocs_.begin(), hallocs_.end(), (void*)h_up_));
      (void)hipFree(d_up_);
      (void)hipHostFree(h_up_);
    }
    up_cap_ = std::max(nd + 4096, 2 * up_cap_);
    d_up_ = dev<PoolUpdate>(up_cap_);
    h_up_ = pinned<PoolUpdate>(up_cap_);
  }
  for (int q = 0; q < nd; q++) {
    if (q + 8 < nd) graph_.prefetch_point(dirty[q + 8]);
    const int h = dirty[q];
    MPoint& p = graph_.mp(h);
    PoolUpdate& u = h_up_[q];
    u.h = h;
    memcpy(u.p.Xw, p.pos, 12);
    memcpy(u.p.normal, p.normal, 12);
    u.p.min_dist = p.minDist;
    u.p.max_dist = p.maxDist;
    u.p.skip = 0;
    memcpy(u.desc, p.desc, 32);
    p.dirty = false;
  }
  MMT_HIP(hipMemcpyAsync(d_up_, h_up_, sizeof(PoolUpdate) * (size_t)nd, hipMemcpyHostToDevice,
                         st));
  launch_pool_scatter(d_up_, nd, d_pool_, d_pool_desc_, st);
  graph_.dirty_flushed();
}

// ------------------------------------------------------------------ Tracking
void MapEngine::initialize(MapFrameH& C, const float* Tcw) {
  const int kf = graph_.new_keyframe(C, Tcw);
  kf_store_add(kf);
  for (int i = 0; i < C.n; i++) {
    const float z = C.depth[i];
    if (z > 0) {
      float x3D[3];
      unproject(cam_, Tcw, C.kps[i].x, C.kps[i].y, z, x3D);
      const int h = graph_.new_point_kf(x3D, kf);
      graph_.add_observation(h, kf, i);
      graph_.kf_set_mp(kf, i, h);
      graph_.compute_distinctive(h);
      graph_.update_normal_depth(h);
      C.mps[i] = h;
    }
  }
  process_new_keyframe(kf);
  map_point_culling(kf);
  local_mapping(kf);  // keyframe 0 never enters the database (LoopClosing.cc:95)
  lastKFFrameId_ = C.id;
  localKFs_.assign(1, kf);
  localPts_.clear();
  for (size_t h = 0; h < graph_.n_points(); h++)
    if (!graph_.mp(h).bad()) localPts_.push_back((int)h);  // mpMap->GetAllMapPoints()
  local_gen_ = lpc_.new_gen();
  refKF_ = kf;
  C.refKF = kf;
  state_ = 1;
}

void MapEngine::frame_done(const MapFrameH& C, const float* Tcw) {
  const int snap = snapKF_;
  snapKF_ = -1;
  if (C.refKF < 0) return;
  // Tcr = mTcw * mpReferenceKF->GetPoseInverse(), with the keyframe's pose as Track() leaves it
  // (before the mapping thread's local BA of a keyframe this frame inserted)
  mat4_mul(Tcw, C.refKF == snap ? snapTwc_ : graph_.kf(C.refKF).Twc, Tlr_);
  hasTlr_ = true;
}

void MapEngine::update_last_frame(MapFrameH& L, float* Tlast) {  // Tracking.cc:2894-2960
  if (L.refKF >= 0 && hasTlr_) mat4_mul(Tlr_, graph_.kf(L.refKF).Tcw, Tlast);
  if (lastKFFrameId_ == L.id) return;
  // The reference sorts (depth, index) and walks the prefix up to the first point that is both
  // beyond thDepth and past the 200th: that prefix is every close point plus the nearest far one,
  // or the 201 nearest points when fewer than 200 are close.  The temporary points are identities
  // only (C2 reads them by key index, they die with the frame), so the set is selected in O(n)
  // instead of sorting the keys.
  auto make = [&](int i) {
    if (L.mps[i] < 0 || graph_.mp(L.mps[i]).nObs() < 1) {
      MPoint p;  // MapPoint(x3D, mpMap, &mLastFrame, i): C2 reads its position and descriptor
      unproject(cam_, Tlast, L.kps[i].x, L.kps[i].y, L.depth[i], p.pos);
      memcpy(p.desc, L.desc + 32 * (size_t)i, 32);
      L.mps[i] = graph_.new_temp_point(p);
    }
  };
  graph_.reserve_temps(L.n);
  far_.clear();
  int nclose = 0;
  for (int i = 0; i < L.n; i++) {
    const float z = L.depth[i];
    if (!(z > 0)) continue;
    if (z > cam_.thDepth) {
      far_.push_back({z, i});
    } else {
      make(i);
      nclose++;
    }
  }
  const size_t need = std::min(far_.size(), (size_t)(nclose >= 200 ? 1 : 201 - nclose));
  if (need == 0) return;
  std::nth_element(far_.begin(), far_.begin() + (need - 1), far_.end());
  for (size_t j = 0; j < need; j++) make(far_[j].second);
}

// TrackWithMotionModel / TrackReferenceKeyFrame's outlier discard: returns nmatches
int MapEngine::discard_outliers(MapFrameH& C, int nmatches, int* nmatchesMap) {
  *nmatchesMap = 0;
  for (int i = 0; i < C.n; i++) {
    if (C.mps[i] < 0) continue;
    if (C.outlier[i]) {
      const int h = C.mps[i];
      MPoint& p = graph_.mp(h);
      C.mps[i] = -1;
      C.outlier[i] = 0;
      p.trackInView = false;
      p.lastSeen = curId_;
      if (h < kTemp) graph_.hot(h).lastSeen = (int)curId_;
      nmatches--;
    } else if (graph_.mp(C.mps[i]).nObs() > 0) {
      (*nmatchesMap)++;
    }
  }
  return nmatches;
}

bool MapEngine::track_with_motion_model(MapFrameH& C, const GridFrame& G, float* Tcw,
                                        MapFrameH& L, float* Tlast, const float* vel,
                                        MapStatsH& st) {
  MAP_PROF(8, update_last_frame(L, Tlast));
  mat4_mul(vel, Tlast, Tcw);
  std::fill(C.mps.begin(), C.mps.end(), -1);
  const float th = 15;
  int nmatches;
  // C2 at th, again at 2 th below 20 matches, then D1 at 20 or more (Tracking.cc:2962-2990)
  MAP_PROF(0, nmatches = gpu_frame_chain(C, G, Tcw, L, Tlast, th, 2 * th, 20, -1, true));
  st.matches_mm = nmatches;
  if (nmatches < 20) return false;
  int nmatchesMap = 0;
  discard_outliers(C, nmatches, &nmatchesMap);
  mbVO_ = nmatchesMap < 20;
  return nmatchesMap >= 10;
}

bool MapEngine::track_reference_subst(MapFrameH& C, const GridFrame& G, float* Tcw,
                                      const MapFrameH& L, const float* Tlast) {
  std::fill(C.mps.begin(), C.mps.end(), -1);
  memcpy(Tcw, Tlast, 64);
  const int nmatches = gpu_frame_chain(C, G, Tcw, L, Tlast, 15, 0, 15);
  if (nmatches < 15) {
    std::fill(C.mps.begin(), C.mps.end(), -1);
    return false;
  }
  int nmatchesMap = 0;
  discard_outliers(C, nmatches, &nmatchesMap);
  return nmatchesMap >= 10;
}

// Relocalization substitute (pinned deviation, as oracle/map_ref.cpp relocalization_subst): the
// reference keyframe and its best 10 covisibles as candidates, each searched as TrackWithMotionModel
// searches the last frame (the keyframe as the last frame, th 15, again at 30 below 20 matches, at
// the pose the motion model predicts from the last, flow-tracked, frame), then the reference's
// acceptance of Tracking.cc:3700-3770 (PoseOptimization: fewer than 10 inliers -> next candidate;
// outliers dropped; 50 inliers or more -> relocalised).
bool MapEngine::relocalization_subst(MapFrameH& C, const GridFrame& G, float* Tcw,
                                     const float* Tlast, const float* vel) {
  std::vector<int> cand;
  if (refKF_ >= 0 && !graph_.kf(refKF_).bad()) cand.push_back(refKF_);
  if (refKF_ >= 0) {
    const std::vector<int>& o = graph_.kf(refKF_).ordered();
    for (size_t q = 0; q < o.size() && q < 10; q++)
      if (!graph_.kf(o[q]).bad()) cand.push_back(o[q]);
  }
  float Tpred[16];
  mat4_mul(vel, Tlast, Tpred);
  for (int k : cand) {
    const KFrame& K = graph_.kf(k);
    MapFrameH V;  // the keyframe as a last frame: its good map points, no outliers
    V.id = K.frameId;
    V.n = (int)K.keys.size();
    V.kps = K.keys.data();
    V.desc = K.desc.data();
    V.uR = K.uR.data();
    V.depth = K.depth.data();
    V.mps = K.mps();
    for (int& h : V.mps)
      if (h >= 0 && graph_.mp(h).bad()) h = -1;
    V.outlier.assign(V.mps.size(), 0);
    memcpy(Tcw, Tpred, 64);
    const int nm = gpu_frame_chain(C, G, Tcw, V, K.Tcw, 15, 30, 15, 20);
    if (nm < 15) continue;
    int nGood = 0;
    for (int i = 0; i < C.n; i++) nGood += C.mps[i] >= 0 && !C.outlier[i];
    if (nGood < 10) continue;
    for (int i = 0; i < C.n; i++)
      if (C.mps[i] >= 0 && C.outlier[i]) {
        C.mps[i] = -1;
        C.outlier[i] = 0;
      }
    if (nGood >= 50) return true;
  }
  std::fill(C.mps.begin(), C.mps.end(), -1);
  memcpy(Tcw, Tpred, 64);
  return false;
}

void MapEngine::update_local_keyframes(MapFrameH& C) {  // Tracking::UpdateLocalKeyFrames
  // keyframeCounter (a std::map keyed by KeyFrame*, here by keyframe id): counts in a flat array,
  // then the touched ids in ascending order, as the map would iterate them
  if (kf_count_.size() < graph_.n_kfs()) kf_count_.resize(graph_.n_kfs(), 0);
  kf_touched_.clear();
  for (int i = 0; i < C.n; i++) {
    if (C.mps[i] < 0) continue;
    const MPoint& p = graph_.mp(C.mps[i]);
    if (!p.bad()) {
      for (const auto& kv : p.obs())
        if (kf_count_[kv.first]++ == 0) kf_touched_.push_back(kv.first);
    } else {
      C.mps[i] = -1;
    }
  }
  if (kf_touched_.empty()) return;
  std::sort(kf_touched_.begin(), kf_touched_.end());
  int mx = 0, kmax = -1;
  localKFs_.clear();
  for (const int id : kf_touched_) {
    const int cnt = kf_count_[id];
    kf_count_[id] = 0;
    KFrame& K = graph_.kf(id);
    if (K.bad()) continue;
    if (cnt > mx) {
      mx = cnt;
      kmax = id;
    }
    localKFs_.push_back(id);
    K.trackRef = curId_;
  }
  graph_.expand_local_kfs(
      localKFs_, [&](int id) { return graph_.kf(id).trackRef == curId_; },
      [&](int id) { graph_.kf(id).trackRef = curId_; });
  if (kmax >= 0) {
    refKF_ = kmax;
    C.refKF = kmax;
  }
}

void MapEngine::update_local_points() { collect_checked(localKFs_, localPts_, local_gen_); }

void MapEngine::collect_checked(const std::vector<int>& kfl, std::vector<int>& out, long& gen) {
  if (!lpc_.collect(graph_, kfl, out, gen))
    throw DeviceError("local point list cache: the cached list differs from the walk's (" +
                      std::to_string(out.size()) + " / " + std::to_string(lpc_.check().size()) +
                      " points, frame " + std::to_string(curId_) + ")");
}

// UpdateLocalMap from C2's final matches while D1 runs (track_with_motion_model; L: the last frame
// whose points the matches index).  Nothing of the map changes between here and TrackLocalMap but
// the frame's bindings, which D1's outliers can only remove: commit_local_map checks that every
// counted keyframe keeps a count (the same keyframe set, so the same expansion and points) and
// recomputes the best-counted keyframe.  Marks are private (spec_mark_), so a speculation that is
// never taken leaves no trace.
void MapEngine::speculate_local_map(const MapFrameH& L, int n) {
  spec_discard();
  const int* match = (const int*)(h_early_ + kOutHdr);
  if (spec_cnt_.size() < graph_.n_kfs()) spec_cnt_.resize(graph_.n_kfs(), 0);
  if (spec_mark_.size() < graph_.n_kfs()) spec_mark_.resize(graph_.n_kfs(), 0);
  spec_mps_.assign(n, -1);
  spec_touched_.clear();
  for (int i = 0; i < n; i++) {
    if (match[i] < 0) continue;
    const int h = L.mps[match[i]];
    spec_mps_[i] = h;
    if (h < 0) continue;
    const MPoint& p = graph_.mp(h);
    if (p.bad()) continue;
    for (const auto& kv : p.obs())
      if (spec_cnt_[kv.first]++ == 0) spec_touched_.push_back(kv.first);
  }
  std::sort(spec_touched_.begin(), spec_touched_.end());
  const long stamp = ++spec_stamp_;
  spec_kfs_.clear();
  for (const int id : spec_touched_)
    if (!graph_.kf(id).bad()) {
      spec_kfs_.push_back(id);
      spec_mark_[id] = stamp;
    }
  spec_frame_ = curId_;
  if (spec_kfs_.empty()) return;  // (the reference's early return keeps the last local map)
  graph_.expand_local_kfs(
      spec_kfs_, [&](int id) { return spec_mark_[id] == stamp; },
      [&](int id) { spec_mark_[id] = stamp; });
  collect_checked(spec_kfs_, spec_pts_, spec_gen_);
  spec_valid_ = true;
  spec_tries_++;
}

void MapEngine::spec_discard() {
  for (const int id : spec_touched_) spec_cnt_[id] = 0;
  spec_touched_.clear();
  spec_valid_ = false;
}

bool MapEngine::commit_local_map(MapFrameH& C) {
  if (!spec_valid_ || spec_frame_ != curId_ || (int)spec_mps_.size() != C.n) {
    spec_discard();
    return false;
  }
  // the bindings now: a subset of the speculated ones; the dropped ones' counts come off
  bool ok = true;
  for (int i = 0; i < C.n && ok; i++) {
    const int h = C.mps[i], s0 = spec_mps_[i];
    if (h >= 0 && h != s0) {
      ok = false;
    } else if (s0 >= 0 && h < 0) {
      const MPoint& p = graph_.mp(s0);
      if (!p.bad())
        for (const auto& kv : p.obs()) spec_cnt_[kv.first]--;
    }
  }
  for (size_t q = 0; q < spec_touched_.size() && ok; q++) {
    const int id = spec_touched_[q];
    ok = graph_.kf(id).bad() || spec_cnt_[id] > 0;
  }
  if (!ok) {
    spec_discard();
    return false;
  }
  for (int i = 0; i < C.n; i++)
    if (C.mps[i] >= 0 && graph_.mp(C.mps[i]).bad()) C.mps[i] = -1;
  int mx = 0, kmax = -1;
  for (const int id : spec_touched_) {
    const int cnt = spec_cnt_[id];
    spec_cnt_[id] = 0;
    if (graph_.kf(id).bad()) continue;
    if (cnt > mx) {
      mx = cnt;
      kmax = id;
    }
  }
  spec_touched_.clear();
  spec_valid_ = false;
  for (const int id : spec_kfs_) graph_.kf(id).trackRef = curId_;
  localKFs_.swap(spec_kfs_);
  localPts_.swap(spec_pts_);
  std::swap(local_gen_, spec_gen_);
  if (kmax >= 0) {
    refKF_ = kmax;
    C.refKF = kmax;
  }
  spec_hits_++;
  return true;
}

void MapEngine::search_local_points(MapFrameH& C, const GridFrame& G, const float* Tcw) {
  const double t_pack = prof_on_ ? now_us() : 0;
  // Tracking::SearchLocalPoints (Tracking.cc:3416-3466)
  for (int i = 0; i < C.n; i++) {
    if (C.mps[i] < 0) continue;
    const int h = C.mps[i];
    MPoint& p = graph_.mp(h);
    if (p.bad()) {
      C.mps[i] = -1;
    } else {
      p.visible++;
      p.lastSeen = curId_;
      if (h < kTemp) graph_.hot(h).lastSeen = (int)curId_;
      p.trackInView = false;
    }
  }
  const int m = (int)localPts_.size();
  grow_local(m);
  gpu_flush_pool();
  // the handles stay on the device while the list is the one uploaded last (its generation); the
  // upload is ordered on s_ behind the previous frame's chain, which has completed (this function
  // ends with a synchronisation), so h_ids_ is free to refill.  MMT_LOCALMAP_CACHE=0: in the
  // upload block, every frame
  const bool ids_inline = lpc_.mode() == 0;
  const SelLayout sl(m, C.n, ids_inline);
  const bool ids_new = ids_inline || ids_gen_ != local_gen_;
  int* ids = ids_inline ? (int*)(h_sel_ + sl.ids) : h_ids_;
  const int* d_ids = ids_inline ? (const int*)(d_sel_ + sl.ids) : d_ids_;
  uint8_t* skip = h_sel_ + sl.skip;
  uint8_t* taken = h_sel_ + sl.taken;
  if (ids_new) {
    memcpy(ids, localPts_.data(), 4 * (size_t)m);
    ids_uploads_++;
  }
  for (int j = 0; j < m; j++) {
    const PtHot& q = graph_.hot(localPts_[j]);
    skip[j] = q.lastSeen == (int)curId_ || q.bad();
  }
  // the keys bound before the search: taken (Observations() > 0) and, for D1's edge list, their
  // points' positions
  float* bX = (float*)(h_sel_ + sl.bX);
  uint8_t* bHas = h_sel_ + sl.bHas;
  int nbase = 0;
  for (int i = 0; i < C.n; i++) {
    const int h = C.mps[i];
    taken[i] = 0;
    bHas[i] = h >= 0;
    if (h >= 0) {
      const MPoint& p = graph_.mp(h);
      taken[i] = p.nObs() > 0;
      memcpy(bX + 3 * (size_t)i, p.pos, 12);
      nbase++;
    }
  }
  if (prof_on_) prof_[10] += now_us() - t_pack;
  pose_desc_fill(h_sel_, d_sel_, Tcw);
  MMT_HIP(hipMemcpyAsync(d_sel_, h_sel_, sl.total, hipMemcpyHostToDevice, s_));
  if (!ids_inline && ids_new) {
    if (m > 0) MMT_HIP(hipMemcpyAsync(d_ids_, h_ids_, 4 * (size_t)m, hipMemcpyHostToDevice, s_));
    ids_gen_ = local_gen_;
  }
  // ORBmatcher(0.8)::SearchByProjection's th: 3 for RGB-D, 5 right after a relocalisation
  const float th = curId_ < lastRelocFrameId_ + 2 ? 5.f : 3.f;
  LocalSel sel{d_ids, d_sel_ + sl.skip, d_inview_};
  // D1 over every key bound after the search (Tracking.cc:3189-3200), chained on the device: the
  // matcher kernel builds its edge list from the final bindings
  MapEdgeArgs e = edge_args(G);
  e.pool = d_pool_;
  e.ids = d_ids;
  e.has_base = d_sel_ + sl.bHas;
  e.base_X = (const float*)(d_sel_ + sl.bX);
  launch_search_local(G, Tcw, d_pool_, d_pool_desc_, m, th, d_sel_ + sl.taken, nullptr, c3_,
                      d_match_, d_nm_, s_, &sel, &e);
  launch_pose_opt(d_pod_, 1, std::min(C.n, nbase + m), s_);
  MMT_HIP(hipMemcpyAsync(h_out_, d_out_, out_bytes(C.n), hipMemcpyDeviceToHost, s_));
  if (m > 0) MMT_HIP(hipMemcpyAsync(h_inview_, d_inview_, (size_t)m, hipMemcpyDeviceToHost, s_));
  // what the hook enqueues (the flow solve) runs behind D1; the host waits for D1's results only
  if (after_d1_) {
    MMT_HIP(hipEventRecord(ev_d1_, s_));
    after_d1_(d_pose_);
  }
  run_overlap();
  if (after_d1_)
    MMT_HIP(hipEventSynchronize(ev_d1_));
  else
    MMT_HIP(hipStreamSynchronize(s_));
  // IncreaseVisible for the points in view (mbTrackInView itself is read by the GPU search only,
  // from h_inview_: the host's copy of the flag is not kept, so only the points in view are touched)
  for (int j = 0; j < m; j++)
    if (!skip[j] && h_inview_[j]) graph_.mp(localPts_[j]).visible++;
  for (int i = 0; i < C.n; i++)
    if (h_match_[i] >= 0) C.mps[i] = localPts_[h_match_[i]];
}

bool MapEngine::track_local_map(MapFrameH& C, const GridFrame& G, float* Tcw) {
  MAP_PROF(2, if (!commit_local_map(C)) {
    update_local_keyframes(C);
    update_local_points();
  });
  if (prof_on_) {
    prof_cnt_[0] += localKFs_.size();
    prof_cnt_[1] += localPts_.size();
  }
  MAP_PROF(3, search_local_points(C, G, Tcw));  // C3, then D1 on the device
  MAP_PROF(4, apply_pose_opt(C, Tcw));
  matchesInliers_ = 0;
  for (int i = 0; i < C.n; i++) {
    if (C.mps[i] < 0 || C.outlier[i]) continue;
    MPoint& p = graph_.mp(C.mps[i]);
    p.found++;
    if (p.nObs() > 0) matchesInliers_++;
  }
  if (curId_ < lastRelocFrameId_ + cam_.maxFrames && matchesInliers_ < 50) return false;
  return matchesInliers_ >= 30;
}

bool MapEngine::need_new_keyframe(const MapFrameH& C) {  // Tracking::NeedNewKeyFrame (RGB-D)
  const int nKFs = n_keyframes();
  if (curId_ < lastRelocFrameId_ + cam_.maxFrames && nKFs > cam_.maxFrames) return false;
  const int nMinObs = nKFs <= 2 ? 2 : 3;
  const int nRefMatches = graph_.tracked_map_points(refKF_, nMinObs);
  const bool bLocalMappingIdle = true;  // synchronous LocalMapping (pinned)
  int nNonTrackedClose = 0, nTrackedClose = 0;
  for (int i = 0; i < C.n; i++)
    if (C.depth[i] > 0 && C.depth[i] < cam_.thDepth) {
      if (C.mps[i] >= 0 && !C.outlier[i])
        nTrackedClose++;
      else
        nNonTrackedClose++;
    }
  const bool bNeedToInsertClose = (nTrackedClose < 100) && (nNonTrackedClose > 70);
  const float thRefRatio = nKFs < 2 ? 0.4f : 0.75f;
  const bool c1a = curId_ >= lastKFFrameId_ + cam_.maxFrames;
  const bool c1b = curId_ >= lastKFFrameId_ && bLocalMappingIdle;
  const bool c1c = matchesInliers_ < nRefMatches * 0.25 || bNeedToInsertClose;
  const bool c2 = (matchesInliers_ < nRefMatches * thRefRatio || bNeedToInsertClose) &&
                  matchesInliers_ > 15;
  return (c1a || c1b || c1c) && c2;
}

void MapEngine::create_new_keyframe(MapFrameH& C, const float* Tcw) {  // Tracking.cc:3333-3414
  double tb = prof_on_ ? now_us() : 0;
  const int kf = graph_.new_keyframe(C, Tcw);
  kf_store_add(kf);
  blk_time(0, tb);
  refKF_ = kf;
  C.refKF = kf;
  // the keys with depth sorted by (depth, index): a stable LSD radix sort on the depths' bits
  // (positive floats order as their bit patterns) over the keys in index order, 3 x 11 bits
  std::vector<uint32_t>& key = sort_key_;
  std::vector<int>& v = sort_idx_;
  std::vector<int>& tmp = sort_tmp_;
  key.clear();
  v.clear();
  for (int i = 0; i < C.n; i++)
    if (C.depth[i] > 0) {
      uint32_t b;
      memcpy(&b, &C.depth[i], 4);
      key.push_back(b);
      v.push_back(i);
    }
  if (!v.empty()) {
    const int nv = (int)v.size();
    std::vector<int> pos(nv);  // position of each entry's key
    for (int k = 0; k < nv; k++) pos[k] = k;
    tmp.resize(nv);
    for (int pass = 0; pass < 3; pass++) {
      uint32_t cnt[2049];
      memset(cnt, 0, sizeof(cnt));
      const int sh = 11 * pass;
      for (int k = 0; k < nv; k++) cnt[((key[pos[k]] >> sh) & 0x7FF) + 1]++;
      for (int b = 0; b < 2048; b++) cnt[b + 1] += cnt[b];
      for (int k = 0; k < nv; k++) tmp[cnt[(key[pos[k]] >> sh) & 0x7FF]++] = pos[k];
      pos.swap(tmp);
    }
    int nPoints = 0;
    for (int j = 0; j < nv; j++) {
      const int i = v[pos[j]];
      const float depth_i = C.depth[i];
      bool create = false;
      if (C.mps[i] < 0) {
        create = true;
      } else if (graph_.mp(C.mps[i]).nObs() < 1) {
        create = true;
        C.mps[i] = -1;
      }
      if (create) {
        float x3D[3];
        unproject(cam_, Tcw, C.kps[i].x, C.kps[i].y, C.depth[i], x3D);
        const int h = graph_.new_point_kf(x3D, kf);
        graph_.add_observation(h, kf, i);
        graph_.kf_set_mp(kf, i, h);
        graph_.compute_distinctive(h);
        graph_.update_normal_depth(h);
        C.mps[i] = h;
      }
      nPoints++;
      if (depth_i > cam_.thDepth && nPoints > 200) break;
    }
  }
  blk_time(1, tb);
  snapKF_ = kf;
  memcpy(snapTwc_, graph_.kf(kf).Twc, sizeof(snapTwc_));
  const double tp = prof_on_ ? now_us() : 0;
  process_new_keyframe(kf);  // mpLocalMapper->InsertKeyFrame(pKF), processed at once
  map_point_culling(kf);
  if (prof_on_) mstats_.pnk_us += now_us() - tp;
  local_mapping(kf);
  // mpLoopCloser->InsertKeyFrame: LoopClosing::DetectLoop adds every keyframe but the first to
  // the database (LoopClosing.cc:92-121); loop detection itself is out of scope
  if (voc_ && graph_.kf(kf).id != 0 && !graph_.kf(kf).bad()) kfdb_add(kf);
  lastKFFrameId_ = C.id;
}

int MapEngine::track(MapFrameH& C, const GridFrame& G, float* Tcw, MapFrameH& L, float* Tlast,
                     float* vel, bool& has_vel, bool& bSecondFrame, MapStatsH& st,
                     hipStream_t s) {
  s_ = s;
  curId_ = C.id;
  const double t_track = prof_on_ ? now_us() : 0;
  bool bOK;
  // a branch that computes no pose leaves the motion model's prediction, or the last pose
  // (pinned as in the oracle: the reference's mCurrentFrame.mTcw stays empty there)
  if (has_vel)
    mat4_mul(vel, Tlast, Tcw);
  else
    memcpy(Tcw, Tlast, 64);
  if (state_ == 1) {
    // CheckReplacedInLastFrame (Tracking.cc:2766-2781): one level of MapPoint::GetReplaced
    for (int i = 0; i < L.n; i++)
      if (L.mps[i] >= 0 && L.mps[i] < kTemp && graph_.mp(L.mps[i]).replaced() >= 0)
        L.mps[i] = graph_.mp(L.mps[i]).replaced();
    if (!has_vel || C.id < lastRelocFrameId_ + 2) {
      bSecondFrame = true;
      bOK = voc_ ? track_reference_kf(C, G, Tcw, Tlast) : track_reference_subst(C, G, Tcw, L, Tlast);
    } else {
      bSecondFrame = false;
      bOK = track_with_motion_model(C, G, Tcw, L, Tlast, vel, st);
      if (!bOK) {
        bSecondFrame = true;
        bOK = voc_ ? track_reference_kf(C, G, Tcw, Tlast)
                   : track_reference_subst(C, G, Tcw, L, Tlast);
      }
    }
  } else if (voc_) {  // Relocalization (Tracking.cc:3614-3776)
    bOK = relocalization(C, G, Tcw);  // from the prediction set above
    if (bOK) lastRelocFrameId_ = C.id;
  } else {
    bOK = relocalization_subst(C, G, Tcw, Tlast, vel);  // Relocalization (substitute)
    if (bOK) lastRelocFrameId_ = C.id;
  }
  C.refKF = refKF_;
  if (bOK && !mbVO_) {
    bOK = track_local_map(C, G, Tcw);
    st.inliers_local = matchesInliers_;
  }
  state_ = bOK ? 1 : 2;
  if (bOK) {
    // motion model from the map pose (Tracking.cc:1117-1125): LastTwc = [Rwc, Ow] of mLastFrame
    float LastTwc[16], Ow[3];
    mat4_eye(LastTwc);
    cam_centre(Tlast, Ow);
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) LastTwc[4 * r + c] = Tlast[4 * c + r];
      LastTwc[4 * r + 3] = Ow[r];
    }
    mat4_mul(Tcw, LastTwc, vel);
    has_vel = true;
  }
  pending_ok_ = bOK;
  if (prof_on_) {
    prof_[7] += now_us() - t_track;
    prof_n_++;
  }
  if (state_ == 2 && n_keyframes() <= 5) return 1;  // mpSystem->Reset(); return
  return 0;
}

void MapEngine::track_finish(MapFrameH& C, MapFrameH& L, const float* Tcw, MapStatsH& st) {
  const double t0 = prof_on_ ? now_us() : 0;
  if (pending_ok_) {
    for (int i = 0; i < C.n; i++)  // clean VO matches
      if (C.mps[i] >= 0 && graph_.mp(C.mps[i]).nObs() < 1) {
        C.outlier[i] = 0;
        C.mps[i] = -1;
      }
    for (int i = 0; i < L.n; i++)  // delete temporal MapPoints (mLastFrame's become dangling)
      if (L.mps[i] >= kTemp) L.mps[i] = -1;
    graph_.clear_temps();
    MAP_PROF(5, if (need_new_keyframe(C)) {
      const double tk = prof_on_ ? now_us() : 0;
      create_new_keyframe(C, Tcw);
      if (prof_on_) mstats_.kfnew_us += now_us() - tk;
      st.new_keyframe = 1;
    });
    for (int i = 0; i < C.n; i++)
      if (C.mps[i] >= 0 && C.outlier[i]) C.mps[i] = -1;
  }
  pending_ok_ = false;
  if (C.refKF < 0) C.refKF = refKF_;
  if (prof_on_) {
    prof_[7] += now_us() - t0;
    prof_[6] = prof_[7];
    for (int k = 0; k < 6; k++) prof_[6] -= prof_[k];
    prof_[6] -= prof_[8];
  }
}

}  // namespace mmt
