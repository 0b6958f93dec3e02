// multimot_track_amd/csrc/mmt_capi_probes.hip -- the C-ABI's matcher and solver probes
// (include/mmt.h): one matcher, solver or transform of the tracking path run alone on host arrays,
// for the parity tests and for callers that keep their own map.  Device memory lives for the call
// (DevBuf); every entry point goes through guard (mmt_ctx.h).

#include <hip/hip_runtime.h>

#include <cstdint>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "mmt_ctx.h"
#include "mmt_devbuf.h"
#include "mmt_mat4.h"
#include "mmt_match.h"
#include "mmt_pnp.h"
#include "mmt_sim3.h"
#include "mmt_sim3opt.h"
#include "mmt_track.h"

using mmt::ArgError;
using mmt::DevBuf;
using mmt::DeviceError;

// The staging blocks of a vocabulary-path matcher probe (MapEngine's own on the tracking path).
struct ProbeStage : mmt::Stage {
  uint8_t* d = nullptr;
  std::vector<uint8_t> h;
  ~ProbeStage() override { (void)hipFree(d); }
  mmt::StageBuf grow(size_t need) override {
    if (need > h.size() || !d) {
      (void)hipFree(d);
      d = nullptr;
      MMT_HIP(hipMalloc((void**)&d, std::max<size_t>(need, 16)));
      h.assign(std::max<size_t>(need, 16), 0);
    }
    return mmt::StageBuf{d, h.data()};
  }
};

// The current frame of a matcher probe on the device: keys, descriptors, depth map, and the B3
// outputs (uR, depth, grid) built by k_stereo_grid.
struct DevMatchFrame {
  int n;
  DevBuf<mmt_kp> kps;
  DevBuf<uint8_t> desc;
  DevBuf<float> depth, uR, kdepth;
  DevBuf<int> nk, cell_start, cell_idx;
  mmt::GridFrame G;
  DevMatchFrame(mmt_ctx* ctx, const mmt_match_frame* cur, bool need_desc)
      : n(cur->n), kps(cur->n), desc(32 * (size_t)cur->n),
        depth((size_t)ctx->cfg.width * ctx->cfg.height), uR(cur->n), kdepth(cur->n), nk(1),
        cell_start(mmt::kGridCells + 1), cell_idx(cur->n) {
    const mmt_config& c = ctx->cfg;
    hipStream_t s = ctx->stream;
    kps.up(cur->kps, n, s);
    if (need_desc) desc.up(cur->desc, 32 * (size_t)n, s);
    depth.up(cur->depth, (size_t)c.width * c.height, s);
    nk.up(&n, 1, s);
    memset(&G, 0, sizeof(G));
    G.keys = kps.p;
    G.desc = desc.p;
    G.uR = uR.p;
    G.cell_start = cell_start.p;
    G.cell_idx = cell_idx.p;
    G.n = n;
    G.fx = c.fx; G.fy = c.fy; G.cx = c.cx; G.cy = c.cy; G.bf = c.bf;
    // Frame::ComputeImageBounds without distortion + grid element sizes (Frame.cc:581-584, 841-846)
    G.minX = 0.0f; G.maxX = (float)c.width; G.minY = 0.0f; G.maxY = (float)c.height;
    G.invW = static_cast<float>(mmt::kGridCols) / static_cast<float>(G.maxX - G.minX);
    G.invH = static_cast<float>(mmt::kGridRows) / static_cast<float>(G.maxY - G.minY);
    G.nlevels = ctx->orb.nlevels;
    for (int l = 0; l < G.nlevels && l < mmt::kMaxLevels; l++) G.scale[l] = ctx->orb.scale[l];
    // mfLogScaleFactor = log(mfScaleFactor), pinned as log in double rounded to float
    G.logScale = (float)std::log((double)ctx->orb.scale[G.nlevels > 1 ? 1 : 0]);
    mmt::launch_stereo_grid(kps.p, nk.p, std::max(n, 1), depth.p, (size_t)c.width * c.height,
                            c.width, c.height, c.bf, G.invW, G.invH, uR.p, kdepth.p,
                            cell_start.p, cell_idx.p, 1, s);
  }
};

static void check_match_frame(mmt_ctx* ctx, const mmt_match_frame* cur, bool need_desc) {
  if (!cur || cur->n < 0 || cur->n > mmt::kMaxMatchKeys) throw ArgError("bad current frame");
  if (cur->n > 0 && (!cur->kps || (need_desc && !cur->desc))) throw ArgError("null frame arrays");
  if (!cur->depth) throw ArgError("null depth map");
  if (ctx->orb.nlevels > mmt::kMaxLevels) throw ArgError("too many pyramid levels");
  const int W = ctx->cfg.width, H = ctx->cfg.height;
  for (int i = 0; i < cur->n; i++) {
    const mmt_kp& k = cur->kps[i];
    if (!(k.x >= 0 && k.y >= 0 && (int)k.x < W && (int)k.y < H))
      throw ArgError("keypoint outside the image");
    if (k.octave < 0 || k.octave >= ctx->orb.nlevels) throw ArgError("keypoint octave out of range");
  }
}

struct DevCands {
  DevBuf<uint32_t> key;
  DevBuf<int> idx, n, choice;
  DevBuf<mmt::PointWin> win;
  explicit DevCands(int m)
      : key((size_t)std::max(m, 1) * mmt::kCandK), idx((size_t)std::max(m, 1) * mmt::kCandK),
        n(m), choice(m), win(m) {}
  mmt::CandSet set() { return mmt::CandSet{key.p, idx.p, n.p, win.p, choice.p}; }
};

// The camera record of Fuse and SearchBySim3 from the context and the frame's grid constants, into
// a zeroed c.  invSigma2 is the caller's: SearchBySim3 does not read it and leaves it zero.
static void fill_fuse_cam(const mmt_ctx* ctx, const mmt::GridFrame& G, float th, mmt::FuseCam& c) {
  const mmt_config& cf = ctx->cfg;
  c.fx = cf.fx; c.fy = cf.fy; c.cx = cf.cx; c.cy = cf.cy; c.bf = cf.bf;
  c.W = (float)cf.width;
  c.H = (float)cf.height;
  c.invW = G.invW;
  c.invH = G.invH;
  c.logScale = G.logScale;
  c.th = th;
  c.nlevels = ctx->orb.nlevels;
  for (int l = 0; l < c.nlevels && l < mmt::kMaxLevels; l++) c.scale[l] = ctx->orb.scale[l];
}

// m map points as the matchers read them (at least one record, so data() is never null): position
// and distance range, the normal and the skip flag where the caller has them (null: left zero).
static std::vector<mmt::LocalPointDev> local_points(int m, const float* Xw, const float* normal,
                                                    const float* min_dist, const float* max_dist,
                                                    const uint8_t* skip) {
  std::vector<mmt::LocalPointDev> hp(std::max(m, 1));  // zeroed
  for (int j = 0; j < m; j++) {
    mmt::LocalPointDev& p = hp[j];
    memcpy(p.Xw, Xw + 3 * (size_t)j, sizeof(p.Xw));
    if (normal) memcpy(p.normal, normal + 3 * (size_t)j, sizeof(p.normal));
    p.min_dist = min_dist[j];
    p.max_dist = max_dist[j];
    if (skip) p.skip = skip[j] != 0;
  }
  return hp;
}

// host checks of a feature vector: ascending node ids, monotone starts from 0, features in
// [0, n); `once` (n bytes, optional) rejects a feature listed twice; nodes of at most max_node
static void check_feature_vector(const mmt_feature_vector* v, int n, std::vector<uint8_t>* once,
                                 int max_node) {
  if (v->n_nodes < 0) throw ArgError("negative node count");
  if (v->n_nodes == 0) return;
  if (!v->node_id || !v->node_start || !v->feat) throw ArgError("null feature vector arrays");
  if (v->node_start[0] != 0) throw ArgError("node_start[0] != 0");
  for (int k = 0; k < v->n_nodes; k++) {
    if (k > 0 && !(v->node_id[k - 1] < v->node_id[k])) throw ArgError("node ids not ascending");
    const int a = v->node_start[k], b = v->node_start[k + 1];
    if (b < a) throw ArgError("node_start not monotone");
    if (b - a > max_node) throw ArgError("a vocabulary node holds more than 16384 frame features");
    for (int q = a; q < b; q++) {
      const int f = v->feat[q];
      if (f < 0 || f >= n) throw ArgError("feature index out of range");
      if (once) {
        if ((*once)[f]) throw ArgError("a frame feature is listed in two nodes");
        (*once)[f] = 1;
      }
    }
  }
}

static void check_sft_keyframe(const mmt_sft_keyframe* k) {
  if (k->n < 0 || k->n > mmt::kMaxMatchKeys) throw ArgError("bad keyframe size");
  if (k->n > 0 && (!k->kps || !k->desc || !k->uR || !k->has_mp))
    throw ArgError("null keyframe arrays");
  std::vector<uint8_t> once((size_t)std::max(k->n, 1), 0);
  check_feature_vector(&k->fv, k->n, &once, INT32_MAX);
}

// An output array of a sample-set probe: `cap` elements the kernel may write and a guard behind
// them, all bytes 0xFF before the launch.  down() copies the cap elements out (entries the kernel
// left alone keep the fill) and throws when the guard changed: a write past the capacity.
template <typename T>
struct GuardedOut {
  static constexpr size_t kGuard = 16;
  DevBuf<T> b;
  size_t cap;
  GuardedOut(size_t cap_, hipStream_t s) : b(cap_ + kGuard), cap(cap_) {
    MMT_HIP(hipMemsetAsync(b.p, 0xFF, (cap + kGuard) * sizeof(T), s));
  }
  void down(T* h, hipStream_t s) const {
    uint8_t g[kGuard * sizeof(T)];
    b.down(h, cap, s);
    MMT_HIP(hipMemcpyAsync(g, b.p + cap, sizeof(g), hipMemcpyDeviceToHost, s));
    MMT_HIP(hipStreamSynchronize(s));
    for (uint8_t x : g)
      if (x != 0xFF) throw DeviceError("object front end probe: write past the output capacity");
  }
};

static void check_image(int W, int H) {
  if (W <= 0 || H <= 0 || (int64_t)W * H > (int64_t)1 << 26) throw ArgError("bad image size");
}

extern "C" {

// init_on_device: the initial pose goes to device memory and the descriptor names it (init_dev),
// its by-value copy poisoned; centre_out (3 floats, optional): ObjCentre3D_pre
static int flow_solve_probe(mmt_ctx* ctx, const mmt_flow_problem* pr, bool init_on_device,
                            float* pose_out, int* stats_out, float* centre_out) {
  if (!ctx || !pr || !pose_out || !stats_out || pr->n < 0) return MMT_EINVAL;
  return guard(ctx, [&] {
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    hipStream_t s = ctx->stream;
    const int n = pr->n, cap = std::max(n, 1);
    DevBuf<float2> obs(cap), flow(cap);
    DevBuf<float> depth(cap), pose(16), init(16), centre(3);
    DevBuf<double> scratch(mmt::flow_scratch_doubles(cap));
    DevBuf<int> st(3);
    DevBuf<mmt::FlowSolveDesc> dd(1);
    const int groups = mmt::flow_split_groups(n);
    DevBuf<unsigned long long> gx(groups > 1 ? mmt::kFlowSplitGranules : 1);
    if (groups > 1)
      MMT_HIP(hipMemsetAsync(gx.p, 0, sizeof(unsigned long long) * mmt::kFlowSplitGranules, s));
    obs.up((const float2*)pr->obs, n, s);
    flow.up((const float2*)pr->flow, n, s);
    depth.up(pr->depth, n, s);
    mmt::FlowSolveDesc d;
    memset(&d, 0, sizeof(d));
    d.n = n;
    d.obs = obs.p;
    d.flow = flow.p;
    d.depth = depth.p;
    memcpy(d.Tcw_last, pr->Tcw_last, 64);
    memcpy(d.init, pr->init, 64);
    d.rp_thres = pr->rp_thres;
    d.use_noise = pr->use_noise;
    d.g0 = pr->g0;
    d.max_iters = pr->max_iters;
    d.prior_info = pr->prior_info;
    d.fx = pr->fx; d.fy = pr->fy; d.cx = pr->cx; d.cy = pr->cy;
    d.scratch = scratch.p;
    d.cap = cap;
    d.pose_out = pose.p;
    d.stats = st.p;
    d.gx = gx.p;
    d.gx_seq = 1;
    if (centre_out) d.centre_out = centre.p;
    if (init_on_device) {
      init.up(pr->init, 16, s);
      d.init_dev = init.p;
      memset(d.init, 0xFF, sizeof(d.init));  // NaNs: a solve that read them would show
    }
    dd.up(&d, 1, s);
    pose.up(pr->init, 16, s);
    if (groups > 1)
      mmt::launch_flow_lm_split(dd.p, groups, s);
    else
      mmt::launch_flow_lm(dd.p, 1, n, s);
    pose.down(pose_out, 16, s);
    st.down(stats_out, 3, s);
    if (centre_out) centre.down(centre_out, 3, s);
    MMT_HIP(hipStreamSynchronize(s));
    if (stats_out[2] == 2)
      throw mmt::DeviceError("pose flow solve: the split solve's workgroups were not resident together");
  });
}

int mmt_pose_flow_solve(mmt_ctx* ctx, const mmt_flow_problem* pr, float* pose_out,
                        int* stats_out) {
  return flow_solve_probe(ctx, pr, false, pose_out, stats_out, nullptr);
}

int mmt_pose_flow_solve_init_dev(mmt_ctx* ctx, const mmt_flow_problem* pr, int init_on_device,
                                 float* pose_out, int* stats_out, float* centre_out) {
  return flow_solve_probe(ctx, pr, init_on_device != 0, pose_out, stats_out, centre_out);
}

int mmt_pose_optimization(mmt_ctx* ctx, const mmt_pose_opt_problem* pr, float* pose_out,
                          uint8_t* outlier_out, int* n_inliers) {
  if (!ctx || !pr || !pose_out || !n_inliers || pr->n < 0 ||
      (pr->n > 0 && (!pr->Xw || !pr->obs || !pr->inv_sigma2 || !outlier_out)))
    return MMT_EINVAL;
  return guard(ctx, [&] {
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    hipStream_t s = ctx->stream;
    const int n = pr->n, cap = std::max(n, 1);
    DevBuf<float> X(3 * (size_t)cap), ob(3 * (size_t)cap), s2(cap), pose(16);
    DevBuf<uint8_t> outl(cap);
    DevBuf<int> ninl(1), fsc(n > mmt::kPoseOptMaxEdges ? cap : 1);
    DevBuf<double> esc(n > mmt::kPoseOptMaxEdges ? 3 * (size_t)cap : 1);
    DevBuf<mmt::PoseOptDesc> dd(1);
    X.up(pr->Xw, 3 * (size_t)n, s);
    ob.up(pr->obs, 3 * (size_t)n, s);
    s2.up(pr->inv_sigma2, n, s);
    mmt::PoseOptDesc d;
    memset(&d, 0, sizeof(d));
    d.n = n;
    d.Xw = X.p;
    d.obs = ob.p;
    d.inv_sigma2 = s2.p;
    memcpy(d.Tcw, pr->Tcw, 64);
    d.fx = pr->fx; d.fy = pr->fy; d.cx = pr->cx; d.cy = pr->cy; d.bf = pr->bf;
    d.pose_out = pose.p;
    d.outlier = outl.p;
    d.n_inliers = ninl.p;
    d.e_scratch = esc.p;
    d.f_scratch = fsc.p;
    dd.up(&d, 1, s);
    mmt::launch_pose_opt(dd.p, 1, n, s);
    pose.down(pose_out, 16, s);
    outl.down(outlier_out, n, s);
    ninl.down(n_inliers, 1, s);
    MMT_HIP(hipStreamSynchronize(s));
  });
}

int mmt_frame_grid(mmt_ctx* ctx, const mmt_match_frame* cur, float* uR_out, float* depth_out,
                   int* cell_start, int* cell_idx) {
  if (!ctx || !cur || !cell_start || (cur->n > 0 && (!uR_out || !depth_out || !cell_idx)))
    return MMT_EINVAL;
  return guard(ctx, [&] {
    check_match_frame(ctx, cur, false);
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    hipStream_t s = ctx->stream;
    DevMatchFrame F(ctx, cur, false);
    F.uR.down(uR_out, cur->n, s);
    F.kdepth.down(depth_out, cur->n, s);
    F.cell_start.down(cell_start, mmt::kGridCells + 1, s);
    MMT_HIP(hipStreamSynchronize(s));
    const int total = cell_start[mmt::kGridCells];
    if (total > 0) {
      F.cell_idx.down(cell_idx, total, s);
      MMT_HIP(hipStreamSynchronize(s));
    }
  });
}

int mmt_search_by_projection_frame(mmt_ctx* ctx, const mmt_match_frame* cur,
                                   const mmt_last_frame* last, float th, int mono,
                                   int check_orientation, int32_t* match_out, int* nmatches) {
  if (!ctx || !cur || !last || !nmatches || last->n < 0 || (cur->n > 0 && !match_out) ||
      (last->n > 0 && (!last->kps || !last->Xw || !last->mp_desc || !last->active)))
    return MMT_EINVAL;
  return guard(ctx, [&] {
    check_match_frame(ctx, cur, true);
    for (int i = 0; i < last->n; i++)
      if (last->active[i] && (last->kps[i].octave < 0 || last->kps[i].octave >= ctx->orb.nlevels))
        throw ArgError("last-frame octave out of range");
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    hipStream_t s = ctx->stream;
    DevMatchFrame F(ctx, cur, true);
    const int n1 = last->n;
    DevBuf<mmt_kp> lk(n1);
    DevBuf<float> X(3 * (size_t)std::max(n1, 1));
    DevBuf<uint8_t> md(32 * (size_t)std::max(n1, 1)), act(n1), obs(n1);
    DevBuf<int> match(cur->n), nm(1);
    DevCands cands(n1);
    lk.up(last->kps, n1, s);
    X.up(last->Xw, 3 * (size_t)n1, s);
    md.up(last->mp_desc, 32 * (size_t)n1, s);
    act.up(last->active, n1, s);
    if (last->obs) obs.up(last->obs, n1, s);
    mmt::LastFrameDev L;
    L.keys = lk.p;
    L.Xw = X.p;
    L.mp_desc = md.p;
    L.active = act.p;
    L.obs = last->obs ? obs.p : nullptr;
    L.n = n1;
    memcpy(L.Tcw, last->Tcw, 64);
    mmt::launch_sbp_frame(F.G, cur->Tcw, L, th, mono, check_orientation, cands.set(), match.p,
                          nm.p, s);
    match.down(match_out, cur->n, s);
    nm.down(nmatches, 1, s);
    MMT_HIP(hipStreamSynchronize(s));
  });
}

int mmt_fuse_candidates(mmt_ctx* ctx, const mmt_match_frame* kf, const mmt_local_points* pts,
                        float th, int32_t* best_idx, int32_t* best_dist) {
  if (!ctx || !kf || !pts || pts->m < 0 || (pts->m > 0 && (!best_idx || !best_dist || !pts->Xw ||
                                                           !pts->normal || !pts->min_dist ||
                                                           !pts->max_dist || !pts->desc)))
    return MMT_EINVAL;
  return guard(ctx, [&] {
    check_match_frame(ctx, kf, true);
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    hipStream_t s = ctx->stream;
    DevMatchFrame F(ctx, kf, true);
    const int m = pts->m;
    const std::vector<mmt::LocalPointDev> hp =
        local_points(m, pts->Xw, pts->normal, pts->min_dist, pts->max_dist, nullptr);
    std::vector<mmt::FuseQuery> hq(std::max(m, 1));
    for (int j = 0; j < m; j++) hq[j] = mmt::FuseQuery{0, j};
    mmt::FuseKF K;
    memset(&K, 0, sizeof(K));
    K.g = mmt::KfGrid{F.G.keys, F.G.desc, F.G.cell_start, F.G.cell_idx};
    K.uR = F.G.uR;
    K.n = kf->n;
    memcpy(K.Tcw, kf->Tcw, 64);
    mmt::cam_centre(kf->Tcw, K.Ow);  // KeyFrame::SetPose
    mmt::FuseCam c;
    memset(&c, 0, sizeof(c));
    fill_fuse_cam(ctx, F.G, th, c);
    for (int l = 0; l < c.nlevels && l < mmt::kMaxLevels; l++)
      c.invSigma2[l] = ctx->orb.invSigma2[l];
    DevBuf<mmt::LocalPointDev> dp(m);
    DevBuf<uint8_t> pd(32 * (size_t)std::max(m, 1));
    DevBuf<mmt::FuseKF> dk(1);
    DevBuf<mmt::FuseQuery> dq(m);
    DevBuf<int2> out(m);
    dk.up(&K, 1, s);
    dp.up(hp.data(), m, s);
    pd.up(pts->desc, 32 * (size_t)m, s);
    dq.up(hq.data(), m, s);
    mmt::launch_fuse_cand(dk.p, dq.p, m, dp.p, pd.p, c, out.p, s);
    std::vector<int2> ho(std::max(m, 1));
    out.down(ho.data(), m, s);
    MMT_HIP(hipStreamSynchronize(s));
    for (int j = 0; j < m; j++) {
      best_idx[j] = ho[j].x;
      best_dist[j] = ho[j].y;
    }
  });
}

int mmt_search_by_sim3(mmt_ctx* ctx, const mmt_match_frame* kf1,
                       const mmt_keyframe_points* points1, const uint8_t* skip1,
                       const mmt_match_frame* kf2, const mmt_keyframe_points* points2,
                       const uint8_t* skip2, float s12, const float* R12, const float* t12,
                       float th, const int32_t* matched12_in, int32_t* match_out, int* n_found,
                       int32_t* cand1_out, int32_t* cand2_out) {
  if (!ctx || !kf1 || !kf2 || !points1 || !points2 || !R12 || !t12 || !n_found) return MMT_EINVAL;
  const mmt_match_frame* kf[2] = {kf1, kf2};
  const mmt_keyframe_points* pts[2] = {points1, points2};
  const uint8_t* skip[2] = {skip1, skip2};
  for (int d = 0; d < 2; d++)
    if (pts[d]->m != kf[d]->n || (pts[d]->m > 0 && (!skip[d] || !pts[d]->Xw || !pts[d]->min_dist ||
                                                    !pts[d]->max_dist || !pts[d]->desc)))
      return MMT_EINVAL;
  if (kf1->n > 0 && (!matched12_in || !match_out)) return MMT_EINVAL;
  return guard(ctx, [&] {
    check_match_frame(ctx, kf1, true);
    check_match_frame(ctx, kf2, true);
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    hipStream_t s = ctx->stream;
    const int n[2] = {kf1->n, kf2->n};
    // vbAlreadyMatched1 / 2 (ORBmatcher.cc:1504-1517)
    std::vector<uint8_t> done[2] = {std::vector<uint8_t>(n[0], 0), std::vector<uint8_t>(n[1], 0)};
    for (int i = 0; i < n[0]; i++) {
      const int m = matched12_in[i];
      if (m == -1) continue;
      done[0][i] = 1;
      if (m >= 0 && m < n[1]) done[1][m] = 1;
    }
    DevMatchFrame F1(ctx, kf1, true), F2(ctx, kf2, true);
    const DevMatchFrame* F[2] = {&F1, &F2};
    DevBuf<mmt::LocalPointDev> dp1(n[0]), dp2(n[1]);
    DevBuf<uint8_t> pd1(32 * (size_t)n[0]), pd2(32 * (size_t)n[1]);
    DevBuf<mmt::LocalPointDev>* dp[2] = {&dp1, &dp2};
    DevBuf<uint8_t>* pd[2] = {&pd1, &pd2};
    mmt::Sim3SearchArgs a;
    memset(&a, 0, sizeof(a));
    std::vector<int> hq;
    for (int d = 0; d < 2; d++) {
      // the points' normals and skip flags are not read by the search: skip decides the queries
      const std::vector<mmt::LocalPointDev> hp =
          local_points(n[d], pts[d]->Xw, nullptr, pts[d]->min_dist, pts[d]->max_dist, nullptr);
      for (int j = 0; j < n[d]; j++)
        if (!skip[d][j] && !done[d][j]) hq.push_back(j);
      if (d == 0) a.nq1 = (int)hq.size();
      dp[d]->up_now(hp.data(), n[d]);  // hp ends with this turn of the loop
      pd[d]->up(pts[d]->desc, 32 * (size_t)n[d], s);
      mmt::Sim3SearchKF& K = a.kf[d];
      K.g = mmt::KfGrid{F[d]->G.keys, F[d]->G.desc, F[d]->G.cell_start, F[d]->G.cell_idx};
      K.pts = dp[d]->p;
      K.pdesc = pd[d]->p;
      memcpy(K.Tcw, kf[d]->Tcw, 64);
    }
    a.nq = (int)hq.size();
    // sR12 = s12 R12, sR21 = (1 / s12) R12^T, t21 = -sR21 t12 (ORBmatcher.cc:1494-1496)
    const double inv = 1.0 / (double)s12;
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) {
        a.T[1][4 * r + c] = s12 * R12[3 * r + c];
        a.T[0][4 * r + c] = (float)(inv * (double)R12[3 * c + r]);
      }
      a.T[1][4 * r + 3] = t12[r];
    }
    for (int r = 0; r < 3; r++) {
      double acc = 0;
      for (int k = 0; k < 3; k++) acc += (double)a.T[0][4 * r + k] * (double)t12[k];
      a.T[0][4 * r + 3] = -(float)acc;
    }
    fill_fuse_cam(ctx, F1.G, th, a.cam);
    DevBuf<int> dq(a.nq);
    DevBuf<int2> out(a.nq);
    std::vector<int2> ho(std::max(a.nq, 1));
    if (a.nq > 0) {
      dq.up(hq, s);
      a.q = dq.p;
      a.out = out.p;
      mmt::launch_sim3_search(a, s);
      out.down(ho.data(), a.nq, s);
    }
    MMT_HIP(hipStreamSynchronize(s));
    // vnMatch1 / vnMatch2: bestDist <= TH_HIGH (:1596, :1676), then the agreement pass (:1682-1698)
    std::vector<int32_t> vn[2] = {std::vector<int32_t>(n[0], -1), std::vector<int32_t>(n[1], -1)};
    for (int qi = 0; qi < a.nq; qi++)
      if (ho[qi].x >= 0 && ho[qi].y <= 100) vn[qi < a.nq1 ? 0 : 1][hq[qi]] = ho[qi].x;
    int found = 0;
    for (int i1 = 0; i1 < n[0]; i1++) {
      const int idx2 = vn[0][i1];
      match_out[i1] = -1;
      if (idx2 >= 0 && vn[1][idx2] == i1) {
        match_out[i1] = idx2;
        found++;
      }
    }
    *n_found = found;
    if (cand1_out && n[0] > 0) memcpy(cand1_out, vn[0].data(), 4 * (size_t)n[0]);
    if (cand2_out && n[1] > 0) memcpy(cand2_out, vn[1].data(), 4 * (size_t)n[1]);
  });
}

int mmt_sim3solver_iterate(mmt_ctx* ctx, int n_solvers, const mmt_sim3_problem* problems,
                           const int32_t* const* randi, const int32_t* n_draw_iters,
                           int n_iterations, mmt_sim3_state* states, mmt_sim3_result* results,
                           mmt_sim3_probe* probes) {
  if (!ctx || (n_solvers > 0 && (!problems || !states || !results))) return MMT_EINVAL;
  return guard(ctx, [&] {
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    mmt::sim3solver_iterate_gpu(ctx->stream, n_solvers, problems, randi, n_draw_iters,
                                n_iterations, states, results, probes);
  });
}

int mmt_optimize_sim3(mmt_ctx* ctx, int n_problems, const mmt_sim3_opt_problem* problems,
                      mmt_sim3_opt_result* results) {
  if (!ctx || (n_problems > 0 && (!problems || !results))) return MMT_EINVAL;
  return guard(ctx, [&] {
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    mmt::sim3_optimize_gpu(ctx->stream, n_problems, problems, results);
  });
}

int mmt_local_bundle_adjustment(mmt_ctx* ctx, const mmt_ba_problem* p, float* Tcw_out,
                                float* Xw_out, uint8_t* erase_out, int32_t* stats) {
  if (!ctx || !p || !stats || p->n_kf < 0 || p->n_pt < 0 || p->n_edge < 0 ||
      (p->n_kf > 0 && (!p->Tcw || !p->fixed || !Tcw_out)) ||
      (p->n_pt > 0 && (!p->Xw || !Xw_out)) ||
      (p->n_edge > 0 && (!p->e_pt || !p->e_kf || !p->e_obs || !p->e_inv_sigma2 || !erase_out)))
    return MMT_EINVAL;
  return guard(ctx, [&] {
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    mmt::BAHostProblem P;
    P.n_kf = p->n_kf;
    P.n_pt = p->n_pt;
    P.n_edge = p->n_edge;
    P.Tcw = p->Tcw;
    P.fixed = p->fixed;
    P.Xw = p->Xw;
    P.e_pt = p->e_pt;
    P.e_kf = p->e_kf;
    P.e_obs = p->e_obs;
    P.e_s = p->e_inv_sigma2;
    const mmt_config& c = ctx->cfg;
    P.fx = c.fx; P.fy = c.fy; P.cx = c.cx; P.cy = c.cy; P.bf = c.bf;
    mmt::BARunner& runner = ctx->ba;
    std::vector<float> T(16 * (size_t)std::max(p->n_kf, 1)), X(3 * (size_t)std::max(p->n_pt, 1));
    std::vector<uint8_t> er(std::max(p->n_edge, 1));
    int st[5] = {0, 0, 0, 0, 0};
    runner.run(P, ctx->stream, T.data(), X.data(), er.data(), st);
    if (p->n_kf > 0) memcpy(Tcw_out, T.data(), 64 * (size_t)p->n_kf);
    if (p->n_pt > 0) memcpy(Xw_out, X.data(), 12 * (size_t)p->n_pt);
    if (p->n_edge > 0) memcpy(erase_out, er.data(), (size_t)p->n_edge);
    for (int i = 0; i < 5; i++) stats[i] = st[i];
  });
}

int mmt_bow_transform(mmt_ctx* ctx, const uint8_t* desc, int n, int levelsup, uint32_t* word,
                      double* weight, uint32_t* node) {
  if (!ctx || n < 0 || (n > 0 && (!desc || !word || !weight || !node))) return MMT_EINVAL;
  return guard(ctx, [&] {
    if (!ctx->voc) throw mmt::ArgError("mmt_bow_transform: no vocabulary loaded");
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    if (n == 0) return;
    if (ctx->voc->empty()) {  // TemplatedVocabulary.h:1134: nothing is transformed
      for (int i = 0; i < n; i++) {
        word[i] = 0;
        weight[i] = 0.0;
        node[i] = 0;
      }
      return;
    }
    ctx->voc->upload();
    hipStream_t s = ctx->stream;
    DevBuf<uint8_t> d(32 * (size_t)n);
    DevBuf<uint32_t> w(n), nd(n);
    DevBuf<double> x(n);
    d.up(desc, 32 * (size_t)n, s);
    mmt::launch_bow_transform(ctx->voc->dev, d.p, n, levelsup, w.p, x.p, nd.p, s);
    w.down(word, n, s);
    x.down(weight, n, s);
    nd.down(node, n, s);
    MMT_HIP(hipStreamSynchronize(s));
  });
}

// The probe of k_loop_score (mmt_loop.hip): its records for every stored vector against kf_id's,
// in storage order, and the score Vocabulary::score finishes from the sum.
int mmt_loop_scores(mmt_ctx* ctx, int32_t kf_id, int32_t* common, int32_t* first, double* sum,
                    double* score, int32_t* ids, int cap, int* n_out) {
  if (!ctx || !n_out || cap < 0) return MMT_EINVAL;
  return guard(ctx, [&] {
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    const auto& slots = ctx->loop.table.slots;
    if (ctx->loop.table.find(kf_id) < 0) throw ArgError("mmt_loop_scores: unknown keyframe id");
    const int n = (int)slots.size();
    *n_out = n;
    if (n > cap || !common || !first || !sum || !score || !ids)
      throw ArgError("mmt_loop_scores: output buffer too small");
    const int scoring = ctx->loopdet.scoring();
    const std::vector<mmt::LoopScore>& sc = ctx->loop.score(kf_id, scoring, ctx->stream);
    for (int k = 0; k < n; k++) {
      common[k] = sc[k].common;
      first[k] = sc[k].first;
      sum[k] = sc[k].sum;
      score[k] = mmt::loop_finish_score(sc[k].sum, scoring);
      ids[k] = slots[k].kf_id;
    }
  });
}

int mmt_search_by_bow(mmt_ctx* ctx, const mmt_bow_keyframe* kf, int n_cur, const mmt_kp* cur_kps,
                      const uint8_t* cur_desc, const mmt_feature_vector* cur_fv, float nn_ratio,
                      int check_orientation, int32_t* match_out, int* nmatches) {
  if (!ctx || !kf || !cur_fv || !nmatches || kf->n < 0 || n_cur < 0 ||
      (n_cur > 0 && (!match_out || !cur_kps || !cur_desc)) ||
      (kf->n > 0 && (!kf->kps || !kf->desc || !kf->mp_valid)))
    return MMT_EINVAL;
  return guard(ctx, [&] {
    check_feature_vector(&kf->fv, kf->n, nullptr, INT32_MAX);
    std::vector<uint8_t> once((size_t)std::max(n_cur, 1), 0);
    check_feature_vector(cur_fv, n_cur, &once, mmt::kMaxMatchKeys);
    std::vector<int2> wide;  // the nodes of k_bow_nodes_wide
    if (kf->fv.n_nodes > 0 && cur_fv->n_nodes > 0)
      mmt::bow_wide_pairs(kf->fv.node_id, kf->fv.n_nodes, cur_fv->node_id, cur_fv->node_start,
                          cur_fv->n_nodes, wide);
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    hipStream_t s = ctx->stream;
    const int nk = kf->n, nkn = kf->fv.n_nodes, nfn = cur_fv->n_nodes;
    const int nkfeat = nkn > 0 ? kf->fv.node_start[nkn] : 0;
    const int nffeat = nfn > 0 ? cur_fv->node_start[nfn] : 0;
    DevBuf<mmt_kp> kk(nk), fk(n_cur);
    DevBuf<uint8_t> kd(32 * (size_t)nk), ok(nk), fd(32 * (size_t)n_cur);
    DevBuf<uint32_t> kn(nkn), fnode(nfn);
    DevBuf<int> ks(nkn + 1), kfe(nkfeat), fs(nfn + 1), ffe(nffeat);
    DevBuf<int> match(n_cur), hist(32), cnt(2);
    DevBuf<int2> wd(wide.size());
    wd.up(wide, s);
    kk.up(kf->kps, nk, s);
    kd.up(kf->desc, 32 * (size_t)nk, s);
    ok.up(kf->mp_valid, nk, s);
    fk.up(cur_kps, n_cur, s);
    fd.up(cur_desc, 32 * (size_t)n_cur, s);
    if (nkn > 0) {
      kn.up(kf->fv.node_id, nkn, s);
      ks.up(kf->fv.node_start, (size_t)nkn + 1, s);
      kfe.up(kf->fv.feat, nkfeat, s);
    }
    if (nfn > 0) {
      fnode.up(cur_fv->node_id, nfn, s);
      fs.up(cur_fv->node_start, (size_t)nfn + 1, s);
      ffe.up(cur_fv->feat, nffeat, s);
    }
    mmt::BowFeatVec a{nkn, kn.p, ks.p, kfe.p}, b{nfn, fnode.p, fs.p, ffe.p};
    mmt::launch_search_by_bow(a, kk.p, kd.p, ok.p, b, fk.p, fd.p, n_cur, nn_ratio,
                              check_orientation, match.p, hist.p, cnt.p, wd.p, (int)wide.size(),
                              s);
    match.down(match_out, n_cur, s);
    cnt.down(nmatches, 1, s, 1);
    MMT_HIP(hipStreamSynchronize(s));
  });
}

// One keyframe of mmt_search_by_bow_keyframes appended to the staging block h: every array at a
// 16-byte boundary, the angles alone of the keys.
static mmt::BowKfSide stage_bow_keyframe(const mmt_bow_keyframe* k, std::vector<uint8_t>& h) {
  auto put = [&](const void* src, size_t bytes) {
    const size_t off = (h.size() + 15) & ~(size_t)15;
    if (off + bytes > UINT32_MAX) throw ArgError("the keyframes exceed the staging block (4 GiB)");
    h.resize(off + bytes);
    if (bytes > 0) memcpy(h.data() + off, src, bytes);
    return (uint32_t)off;
  };
  mmt::BowKfSide s;
  s.n = k->n;
  s.n_nodes = k->fv.n_nodes;
  std::vector<float> angle((size_t)k->n);
  for (int i = 0; i < k->n; i++) angle[i] = k->kps[i].angle;
  s.angle = put(angle.data(), 4 * (size_t)k->n);
  s.desc = put(k->desc, 32 * (size_t)k->n);
  s.ok = put(k->mp_valid, (size_t)k->n);
  const int nn = k->fv.n_nodes;
  s.node = put(k->fv.node_id, 4 * (size_t)nn);
  s.start = put(k->fv.node_start, nn > 0 ? 4 * ((size_t)nn + 1) : 0);
  s.feat = put(k->fv.feat, nn > 0 ? 4 * (size_t)k->fv.node_start[nn] : 0);
  return s;
}

static void check_bow_keyframe(const mmt_bow_keyframe* k, int max_node) {
  if (k->n < 0) throw ArgError("negative key count");
  if (k->n > 0 && (!k->kps || !k->desc || !k->mp_valid)) throw ArgError("null keyframe arrays");
  std::vector<uint8_t> once((size_t)std::max(k->n, 1), 0);
  check_feature_vector(&k->fv, k->n, &once, max_node);
}

int mmt_search_by_bow_keyframes(mmt_ctx* ctx, const mmt_bow_keyframe* kf1, int n_cand,
                                const mmt_bow_keyframe* kf2, float nn_ratio,
                                int check_orientation, int32_t* match12_out,
                                int32_t* nmatches_out) {
  if (!ctx || !kf1 || n_cand < 0 || (n_cand > 0 && (!kf2 || !nmatches_out))) return MMT_EINVAL;
  return guard(ctx, [&] {
    if (n_cand > 64) throw ArgError("mmt_search_by_bow_keyframes: more than 64 candidates");
    // keyframe 1: a feature listed twice would have two nodes write one match12 slot
    check_bow_keyframe(kf1, INT32_MAX);
    for (int c = 0; c < n_cand; c++) check_bow_keyframe(&kf2[c], mmt::kMaxMatchKeys);
    if (n_cand == 0) return;
    const int n1 = kf1->n;
    if (n1 > 0 && !match12_out) throw ArgError("null match12_out");
    const size_t rows = (size_t)n_cand * (size_t)n1;
    if (n1 == 0 || kf1->fv.n_nodes == 0) {  // nothing is replayed
      for (size_t i = 0; i < rows; i++) match12_out[i] = -1;
      for (int c = 0; c < n_cand; c++) nmatches_out[c] = 0;
      return;
    }
    // the staging block: candidate table, keyframe 1, the candidates, the wide triples
    std::vector<uint8_t> h(sizeof(mmt::BowKfSide) * (size_t)n_cand);
    mmt::BowKfArgs a;
    a.kf1 = stage_bow_keyframe(kf1, h);
    std::vector<int4> wide;
    for (int c = 0; c < n_cand; c++) {
      const mmt::BowKfSide s = stage_bow_keyframe(&kf2[c], h);
      memcpy(h.data() + sizeof(s) * (size_t)c, &s, sizeof(s));
      if (s.n_nodes > 0)
        mmt::bow_kf_wide_triples(c, kf1->fv.node_id, kf1->fv.n_nodes, kf2[c].fv.node_id,
                                 kf2[c].fv.node_start, s.n_nodes, wide);
    }
    const size_t wide_off = (h.size() + 15) & ~(size_t)15;
    h.resize(wide_off + sizeof(int4) * wide.size());
    if (!wide.empty()) memcpy(h.data() + wide_off, wide.data(), sizeof(int4) * wide.size());
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    hipStream_t s = ctx->stream;
    DevBuf<uint8_t> blk(h.size());
    DevBuf<int> out(rows + (size_t)n_cand), scratch(31 * (size_t)n_cand);
    blk.up(h, s);
    a.blk = blk.p;
    a.cand = reinterpret_cast<const mmt::BowKfSide*>(blk.p);
    a.wide = reinterpret_cast<const int4*>(blk.p + wide_off);
    a.n_cand = n_cand;
    a.n_wide = (int)wide.size();
    a.ratio = nn_ratio;
    a.check_orientation = check_orientation;
    a.match12 = out.p;
    a.nmatches = out.p + rows;
    a.hist = scratch.p;
    a.counters = scratch.p + 30 * (size_t)n_cand;
    mmt::launch_search_by_bow_keyframes(a, s);
    std::vector<int> r(rows + (size_t)n_cand);
    out.down(r.data(), r.size(), s);
    MMT_HIP(hipStreamSynchronize(s));
    memcpy(match12_out, r.data(), 4 * rows);
    memcpy(nmatches_out, r.data() + rows, 4 * (size_t)n_cand);
  });
}

int mmt_search_by_projection_keyframe(mmt_ctx* ctx, const mmt_match_frame* cur,
                                      const mmt_keyframe_points* pts, const uint8_t* skip,
                                      float th, int orb_dist, const uint8_t* bound_in,
                                      int32_t* match_out, int* nmatches, int* n_rescan) {
  if (!ctx || !cur || !pts || !nmatches || pts->m < 0 ||
      (cur->n > 0 && (!match_out || !bound_in)) ||
      (pts->m > 0 && (!pts->Xw || !pts->min_dist || !pts->max_dist || !pts->desc ||
                      !pts->angle || !skip)))
    return MMT_EINVAL;
  return guard(ctx, [&] {
    check_match_frame(ctx, cur, true);
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    hipStream_t s = ctx->stream;
    DevMatchFrame F(ctx, cur, true);
    std::vector<mmt::SbpKfPoint> P;
    std::vector<float> angle;
    std::vector<int> src;  // listed point -> index into pts
    for (int j = 0; j < pts->m; j++) {
      if (skip[j]) continue;
      mmt::SbpKfPoint p;
      memset(&p, 0, sizeof(p));
      memcpy(p.Xw, pts->Xw + 3 * (size_t)j, 12);
      p.min_dist = pts->min_dist[j];
      p.max_dist = pts->max_dist[j];
      memcpy(p.desc, pts->desc + 32 * (size_t)j, 32);
      P.push_back(p);
      angle.push_back(pts->angle[j]);
      src.push_back(j);
    }
    ProbeStage stage;
    std::vector<int> match(std::max(cur->n, 1), -1);
    *nmatches = mmt::sbp_kf_flat(F.G, cur->kps, cur->desc, cur->Tcw, P.data(), angle.data(),
                                 (int)P.size(), bound_in, th, orb_dist, match.data(), n_rescan,
                                 stage, s);
    for (int i = 0; i < cur->n; i++) match_out[i] = match[i] >= 0 ? src[match[i]] : -1;
  });
}

int mmt_search_for_triangulation(mmt_ctx* ctx, const mmt_sft_keyframe* kf1, int n_pairs,
                                 const mmt_sft_keyframe* kf2, int32_t* match12_out,
                                 float* F12_out, int* nmatches) {
  if (!ctx || !kf1 || n_pairs < 0 ||
      (n_pairs > 0 && (!kf2 || !F12_out || !nmatches || (kf1->n > 0 && !match12_out))))
    return MMT_EINVAL;
  return guard(ctx, [&] {
    if (ctx->orb.nlevels > mmt::kMaxLevels) throw ArgError("too many pyramid levels");
    check_sft_keyframe(kf1);
    for (int p = 0; p < n_pairs; p++) check_sft_keyframe(kf2 + p);
    auto octaves = [&](const mmt_sft_keyframe* k) {
      for (int i = 0; i < k->n; i++)
        if (k->kps[i].octave < 0 || k->kps[i].octave >= ctx->orb.nlevels)
          throw ArgError("keypoint octave out of range");
    };
    octaves(kf1);
    for (int p = 0; p < n_pairs; p++) octaves(kf2 + p);
    if (n_pairs == 0) return;
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    hipStream_t s = ctx->stream;
    mmt::MapCamH cam;
    cam.fx = ctx->cfg.fx; cam.fy = ctx->cfg.fy; cam.cx = ctx->cfg.cx; cam.cy = ctx->cfg.cy;
    cam.bf = ctx->cfg.bf;
    cam.nlevels = ctx->orb.nlevels;
    cam.scale.assign(ctx->orb.scale.begin(), ctx->orb.scale.end());
    struct DevKF {
      DevBuf<mmt_kp> kps;
      DevBuf<uint8_t> desc;
      DevBuf<float> uR;
      float Ow[3];
      explicit DevKF(int n) : kps(n), desc(32 * (size_t)n), uR(n) {}
    };
    std::vector<std::unique_ptr<DevKF>> dev;
    auto view = [&](const mmt_sft_keyframe* k) {
      dev.emplace_back(new DevKF(k->n));
      DevKF& D = *dev.back();
      D.kps.up(k->kps, k->n, s);
      D.desc.up(k->desc, 32 * (size_t)k->n, s);
      D.uR.up(k->uR, k->n, s);
      mmt::cam_centre(k->Tcw, D.Ow);  // KeyFrame::GetCameraCenter
      mmt::SftKeyFrame v;
      v.n = k->n;
      v.d_keys = D.kps.p;
      v.d_desc = D.desc.p;
      v.d_uR = D.uR.p;
      v.fv = mmt::BowFeatVec{k->fv.n_nodes, k->fv.node_id, k->fv.node_start, k->fv.feat};
      v.has_mp = k->has_mp;
      v.Tcw = k->Tcw;
      v.Ow = D.Ow;
      return v;
    };
    const mmt::SftKeyFrame V1 = view(kf1);
    std::vector<mmt::SftKeyFrame> V2;
    for (int p = 0; p < n_pairs; p++) V2.push_back(view(kf2 + p));
    ProbeStage stage;
    std::vector<int> m12((size_t)n_pairs * (size_t)std::max(kf1->n, 1), -1);
    mmt::sft_flat(cam, V1, n_pairs, V2.data(), m12.data(), F12_out, nmatches, stage, s);
    if (kf1->n > 0) memcpy(match12_out, m12.data(), 4 * (size_t)n_pairs * (size_t)kf1->n);
  });
}

int mmt_search_local_points(mmt_ctx* ctx, const mmt_match_frame* cur,
                            const mmt_local_points* pts, float th, const uint8_t* taken,
                            int32_t* match_out, float* frustum_out, int* nmatches) {
  if (!ctx || !cur || !pts || !nmatches || pts->m < 0 || (cur->n > 0 && !match_out) ||
      (pts->m > 0 && (!pts->Xw || !pts->normal || !pts->min_dist || !pts->max_dist ||
                      !pts->desc || !pts->skip)))
    return MMT_EINVAL;
  return guard(ctx, [&] {
    check_match_frame(ctx, cur, true);
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    hipStream_t s = ctx->stream;
    DevMatchFrame F(ctx, cur, true);
    const int m = pts->m;
    const std::vector<mmt::LocalPointDev> hp =
        local_points(m, pts->Xw, pts->normal, pts->min_dist, pts->max_dist, pts->skip);
    DevBuf<mmt::LocalPointDev> dp(m);
    DevBuf<uint8_t> pd(32 * (size_t)std::max(m, 1)), tk(cur->n);
    DevBuf<mmt::FrustumRec> fr(m);
    DevBuf<int> match(cur->n), nm(1);
    DevCands cands(m);
    dp.up(hp.data(), m, s);
    pd.up(pts->desc, 32 * (size_t)m, s);
    if (taken) tk.up(taken, cur->n, s);
    mmt::launch_search_local(F.G, cur->Tcw, dp.p, pd.p, m, th, taken ? tk.p : nullptr, fr.p,
                             cands.set(), match.p, nm.p, s);
    std::vector<mmt::FrustumRec> hfr(std::max(m, 1));
    match.down(match_out, cur->n, s);
    fr.down(hfr.data(), m, s);
    nm.down(nmatches, 1, s);
    MMT_HIP(hipStreamSynchronize(s));
    if (frustum_out)
      for (int j = 0; j < m; j++) {
        float* o = frustum_out + 6 * (size_t)j;
        o[0] = (float)hfr[j].in_view;
        o[1] = (float)hfr[j].level;
        o[2] = hfr[j].u;
        o[3] = hfr[j].v;
        o[4] = hfr[j].uR;
        o[5] = hfr[j].view_cos;
      }
  });
}

int mmt_pnp_ransac(mmt_ctx* ctx, const float* pts3, const float* pts2, int n, float fx,
                   float fy, float cx, float cy, int max_iters, double reproj, double confidence,
                   double* R_out, double* t_out, int* inliers_out, int* n_inliers,
                   int* iters_out) {
  if (!ctx || !pts3 || !pts2 || !R_out || !t_out || !n_inliers || !iters_out || n < 5 ||
      max_iters < 1)
    return MMT_EINVAL;
  return guard(ctx, [&] {
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    hipStream_t s = ctx->stream;
    const int words = (n + 63) / 64;
    DevBuf<float> p3(3 * (size_t)n);
    DevBuf<float2> p2(n);
    DevBuf<int> dn(1), sub(5 * (size_t)max_iters), good(max_iters), inl(n), mm(n), subset(n),
        nsub(1), res(8);
    DevBuf<double> models(6 * (size_t)max_iters), Rt(12);
    DevBuf<double> hrec((size_t)mmt::kHypRec * max_iters), hout((size_t)3 * mmt::kHypOut * max_iters);
    DevBuf<unsigned long long> masks((size_t)max_iters * words);
    DevBuf<mmt::PnPObject> po(1);
    std::vector<int> h_sub;
    mmt::ransac_subsets(n, max_iters, h_sub);
    p3.up(pts3, 3 * (size_t)n, s);
    p2.up((const float2*)pts2, n, s);
    dn.up(&n, 1, s);
    sub.up(h_sub, s);
    mmt::PnPObject o;
    memset(&o, 0, sizeof(o));
    o.n = dn.p;
    o.fx = fx; o.fy = fy; o.cx = cx; o.cy = cy;
    o.reproj = reproj;
    o.confidence = confidence;
    o.subsets = sub.p;
    o.pts3 = p3.p;
    o.pts2 = p2.p;
    o.models = models.p;
    o.hrec = hrec.p;
    o.hout = hout.p;
    o.good = good.p;
    o.masks = masks.p;
    o.mask_words = words;
    o.inliers = inl.p;
    o.mm_inliers = mm.p;
    o.subset = subset.p;
    o.n_subset = nsub.p;
    o.result = res.p;
    o.Rt = Rt.p;
    po.up(&o, 1, s);
    mmt::launch_pnp(po.p, 1, max_iters, s, false);
    int r[8];
    double rt[12];
    res.down(r, 8, s);
    Rt.down(rt, 12, s);
    MMT_HIP(hipStreamSynchronize(s));
    const int ni = r[0] >= 0 ? r[3] : 0;
    if (inliers_out && ni > 0) inl.down_now(inliers_out, ni);
    memcpy(R_out, rt, 72);
    memcpy(t_out, rt + 9, 24);
    *n_inliers = ni;
    iters_out[0] = r[2];
    iters_out[1] = r[0];
  });
}

int mmt_pnpsolver_iterate(mmt_ctx* ctx, const mmt_pnpsolver_problem* pr, const int32_t* randi,
                          int n_draw_iters, int n_iterations, mmt_pnpsolver_state* st,
                          float* Tcw_out, uint8_t* inliers_out, int* n_inliers, int* pose_found,
                          int* no_more) {
  if (!ctx || !pr || !st || !Tcw_out || !inliers_out || !n_inliers || !pose_found || !no_more ||
      pr->n < 0 || !st->best_mask || n_iterations < 0 || n_draw_iters < 0)
    return MMT_EINVAL;
  if (pr->n > 0 && (!pr->pts3 || !pr->pts2 || !pr->sigma2)) return MMT_EINVAL;
  return guard(ctx, [&] {
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    mmt::pnpsolver_iterate_gpu(ctx->stream, pr, randi, n_draw_iters, n_iterations, st, Tcw_out,
                               inliers_out, n_inliers, pose_found, no_more);
  });
}

// ---- object front end probes (A2, B1, B2, B4, B6 + B7 statistics)
int mmt_gray_depth(mmt_ctx* ctx, const uint8_t* bgr, size_t bgr_pitch, const uint16_t* disp,
                   size_t disp_pitch, int npix, int nframes, float bf, uint8_t* gray,
                   size_t gray_pitch, float* depth, size_t depth_pitch) {
  if (!ctx || !bgr || !disp || !gray || !depth) return MMT_EINVAL;
  return guard(ctx, [&] {
    if (npix <= 0 || npix > 1 << 26 || nframes <= 0 || nframes > 64)
      throw ArgError("bad pixel or frame count");
    if (bgr_pitch < 3 * (size_t)npix || disp_pitch < (size_t)npix || gray_pitch < (size_t)npix ||
        depth_pitch < (size_t)npix)
      throw ArgError("frame pitch below the frame size");
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    hipStream_t s = ctx->stream;
    const size_t nf = (size_t)nframes;
    DevBuf<uint8_t> B(nf * bgr_pitch), G(nf * gray_pitch);
    DevBuf<uint16_t> D(nf * disp_pitch);
    DevBuf<float> Z(nf * depth_pitch);
    B.up(bgr, nf * bgr_pitch, s);
    D.up(disp, nf * disp_pitch, s);
    G.up(gray, nf * gray_pitch, s);  // the outputs' padding keeps the caller's bytes
    Z.up(depth, nf * depth_pitch, s);
    mmt::launch_gray_depth(B.p, bgr_pitch, D.p, disp_pitch, G.p, gray_pitch, Z.p, depth_pitch,
                           npix, nframes, bf, s);
    G.down(gray, nf * gray_pitch, s);
    Z.down(depth, nf * depth_pitch, s);
    MMT_HIP(hipStreamSynchronize(s));
  });
}

int mmt_static_samples(mmt_ctx* ctx, const mmt_kp* kps, int n, const float* depth,
                       const float* flow, const int32_t* mask, int W, int H, int cap,
                       float* keys_out, float* corres_out, float* flow_out, float* depth_out,
                       int* count) {
  if (!ctx || !depth || !flow || !mask || !keys_out || !corres_out || !flow_out || !depth_out ||
      !count || n < 0 || (n > 0 && !kps) || cap < 0)
    return MMT_EINVAL;
  return guard(ctx, [&] {
    check_image(W, H);
    for (int i = 0; i < n; i++)  // the kernel reads the maps at the truncated key, unchecked
      if (!(kps[i].x >= 0 && kps[i].y >= 0 && (int)kps[i].x < W && (int)kps[i].y < H))
        throw ArgError("keypoint outside the image");
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    hipStream_t s = ctx->stream;
    const size_t np = (size_t)W * H;
    DevBuf<mmt_kp> K(n);
    DevBuf<int> nk(1), cnt(1);
    DevBuf<float> Z(np);
    DevBuf<float2> F(np);
    DevBuf<int32_t> M(np);
    GuardedOut<float2> ok(cap, s), oc(cap, s), of(cap, s);
    GuardedOut<float> od(cap, s);
    K.up(kps, n, s);
    nk.up(&n, 1, s);
    Z.up(depth, np, s);
    F.up((const float2*)flow, np, s);
    M.up(mask, np, s);
    mmt::SampleSet out{ok.b.p, oc.b.p, of.b.p, od.b.p, cnt.p, cap};
    mmt::launch_static_samples(K.p, nk.p, Z.p, F.p, M.p, W, H, out, s);
    cnt.down(count, 1, s);
    ok.down((float2*)keys_out, s);
    oc.down((float2*)corres_out, s);
    of.down((float2*)flow_out, s);
    od.down(depth_out, s);
  });
}

int mmt_object_samples(mmt_ctx* ctx, const float* depth, const float* flow, const int32_t* mask,
                       int W, int H, int cap, float* keys_out, float* corres_out, float* flow_out,
                       float* depth_out, int32_t* label_out, int* count) {
  if (!ctx || !depth || !flow || !mask || !keys_out || !corres_out || !flow_out || !depth_out ||
      !label_out || !count || cap < 0)
    return MMT_EINVAL;
  return guard(ctx, [&] {
    check_image(W, H);
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    hipStream_t s = ctx->stream;
    const size_t np = (size_t)W * H;
    DevBuf<int> cnt(1), blocks(64);
    DevBuf<float> Z(np);
    DevBuf<float2> F(np);
    DevBuf<int32_t> M(np);
    GuardedOut<float2> ok(cap, s), oc(cap, s), of(cap, s);
    GuardedOut<float> od(cap, s);
    GuardedOut<int32_t> ol(cap, s);
    Z.up(depth, np, s);
    F.up((const float2*)flow, np, s);
    M.up(mask, np, s);
    mmt::ObjSampleSet out{ok.b.p, oc.b.p, of.b.p, od.b.p, ol.b.p, cnt.p, cap, blocks.p};
    mmt::launch_obj_samples(Z.p, F.p, M.p, W, H, out, s);
    cnt.down(count, 1, s);
    ok.down((float2*)keys_out, s);
    oc.down((float2*)corres_out, s);
    of.down((float2*)flow_out, s);
    od.down(depth_out, s);
    ol.down(label_out, s);
  });
}

int mmt_sample_handoff(mmt_ctx* ctx, const float* last_corres, int ns, const float* last_obj_corres,
                       int no, const float* depth, const int32_t* mask, int W, int H,
                       float* skeys_out, float* sdepth_out, float* okeys_out, float* odepth_out,
                       int32_t* olabel_out, int* ns_out, int* no_out) {
  if (!ctx || !depth || !mask || !ns_out || !no_out || ns < 0 || no < 0 ||
      (ns > 0 && (!last_corres || !skeys_out || !sdepth_out)) ||
      (no > 0 && (!last_obj_corres || !okeys_out || !odepth_out || !olabel_out)))
    return MMT_EINVAL;
  return guard(ctx, [&] {
    check_image(W, H);
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    hipStream_t s = ctx->stream;
    const size_t np = (size_t)W * H;
    DevBuf<float2> lc(ns), loc(no);
    DevBuf<int> dn(4);
    DevBuf<float> Z(np);
    DevBuf<int32_t> M(np);
    GuardedOut<float2> sk(ns, s), okk(no, s);
    GuardedOut<float> sd(ns, s), od(no, s);
    GuardedOut<int32_t> ol(no, s);
    const int hn[4] = {ns, no, -1, -1};
    lc.up((const float2*)last_corres, ns, s);
    loc.up((const float2*)last_obj_corres, no, s);
    dn.up(hn, 4, s);
    Z.up(depth, np, s);
    M.up(mask, np, s);
    mmt::HandoffSet cur{sk.b.p, sd.b.p, dn.p + 2, okk.b.p, od.b.p, ol.b.p, dn.p + 3};
    mmt::launch_handoff(lc.p, dn.p, loc.p, dn.p + 1, Z.p, M.p, W, H, cur, s);
    int back[4];
    dn.down(back, 4, s);
    if (ns > 0) {
      sk.down((float2*)skeys_out, s);
      sd.down(sdepth_out, s);
    }
    if (no > 0) {
      okk.down((float2*)okeys_out, s);
      od.down(odepth_out, s);
      ol.down(olabel_out, s);
    }
    MMT_HIP(hipStreamSynchronize(s));
    *ns_out = back[2];
    *no_out = back[3];
  });
}

int mmt_object_groups(mmt_ctx* ctx, const mmt_obj_group_problem* pr, int32_t* obj_label_out,
                      int32_t* members_out, int32_t* stats_out, int32_t* hist_out, int* err_out) {
  if (!ctx || !pr || !stats_out || !hist_out || !err_out || pr->n < 0 ||
      (pr->n > 0 && (!pr->cur_keys || !pr->cur_depth || !pr->cur_label || !pr->last_keys ||
                     !pr->last_depth || !pr->last_label || !obj_label_out || !members_out)))
    return MMT_EINVAL;
  static_assert(sizeof(mmt::LabelStats) == 32, "stats_out is 8 words per label");
  return guard(ctx, [&] {
    check_image(pr->W, pr->H);
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    hipStream_t s = ctx->stream;
    const int n = pr->n, mcap = std::max(n, 1);  // member_cap = n, as the tracker's ocap_ >= n
    DevBuf<float2> ck(n), lk(n);
    DevBuf<float> cd(n), ld(n);
    DevBuf<int32_t> cl(n), ll(n);
    DevBuf<int> dn(1), err(1), hist(mmt::kMaxLabel * mmt::kMaxLabel);
    DevBuf<mmt::LabelStats> stats(mmt::kMaxLabel);
    GuardedOut<int32_t> ol(n, s);
    GuardedOut<int> mem((size_t)mmt::kMaxLabel * mcap, s);
    ck.up((const float2*)pr->cur_keys, n, s);
    cd.up(pr->cur_depth, n, s);
    cl.up(pr->cur_label, n, s);
    lk.up((const float2*)pr->last_keys, n, s);
    ld.up(pr->last_depth, n, s);
    ll.up(pr->last_label, n, s);
    dn.up(&n, 1, s);
    MMT_HIP(hipMemsetAsync(err.p, 0, sizeof(int), s));
    MMT_HIP(hipMemsetAsync(stats.p, 0xFF, sizeof(mmt::LabelStats) * mmt::kMaxLabel, s));
    mmt::GroupArgs g;
    memset(&g, 0, sizeof(g));
    g.n = dn.p;
    g.cur_keys = ck.p;
    g.cur_depth = cd.p;
    g.cur_label = cl.p;
    g.last_keys = lk.p;
    g.last_depth = ld.p;
    g.last_label = ll.p;
    memcpy(g.Tcur, pr->Tcur, sizeof(g.Tcur));
    memcpy(g.Tlast, pr->Tlast, sizeof(g.Tlast));
    g.fx = pr->fx; g.fy = pr->fy; g.cx = pr->cx; g.cy = pr->cy;
    g.W = pr->W;
    g.H = pr->H;
    g.obj_label = ol.b.p;
    g.members = mem.b.p;
    g.member_cap = mcap;
    g.stats = stats.p;
    g.hist = hist.p;
    g.err = err.p;
    mmt::launch_obj_group(g, s);
    err.down(err_out, 1, s);
    stats.down((mmt::LabelStats*)stats_out, mmt::kMaxLabel, s);
    hist.down(hist_out, mmt::kMaxLabel * mmt::kMaxLabel, s);
    if (n > 0) {
      ol.down(obj_label_out, s);
      mem.down(members_out, s);
    }
    MMT_HIP(hipStreamSynchronize(s));
    // the flag lives in this call's own buffer: the next call starts clean
    if (*err_out) throw ArgError("semantic label outside [0, 15] on the object path");
  });
}

}  // extern "C"
