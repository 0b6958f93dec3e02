// multimot_track_amd/csrc/mmt_capi.hip -- the C-ABI of libmmt (include/mmt.h): context lifetime,
// ORB extraction, stereo frames, tracking, the vocabulary, counters, dump and debug entry points.
// The matcher and solver probes are in mmt_capi_probes.hip.
// Every entry point catches internal exceptions and returns an errno-style code (guard, mmt_ctx.h);
// nothing exits.

#include <hip/hip_runtime.h>

#include <cstdint>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include <new>

#include "mmt_ctx.h"
#include "mmt_devbuf.h"
#include "mmt_voctrain.h"

using mmt::ArgError;
using mmt::DevBuf;
using mmt::DeviceError;

static thread_local std::string g_create_error;

extern "C" {

int mmt_version(void) { return 100; }

const char* mmt_last_error(const mmt_ctx* ctx) {
  return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

mmt_ctx* mmt_create(const mmt_config* cfg) {
  if (!cfg) {
    g_create_error = "null config";
    return nullptr;
  }
  mmt_ctx* ctx = new (std::nothrow) mmt_ctx();
  if (!ctx) return nullptr;
  ctx->cfg = *cfg;
  try {
    if (cfg->width <= 0 || cfg->height <= 0) throw ArgError("bad image size");
    if (cfg->k1 != 0.f) throw ArgError("distortion must be zero on this path (Frame.cc:789)");
    if (cfg->orb_nlevels < 1 || cfg->orb_nlevels > 16) throw ArgError("bad orb_nlevels");
    if (cfg->orb_nfeatures < 1) throw ArgError("bad orb_nfeatures");
    int ndev = 0;
    MMT_HIP(hipGetDeviceCount(&ndev));
    if (cfg->device_id < 0 || cfg->device_id >= ndev) throw ArgError("bad device_id");
    MMT_HIP(hipSetDevice(cfg->device_id));
    // the context stream (ORB window, ego chain) at normal priority (high measured within noise)
    MMT_HIP(hipStreamCreateWithPriority(&ctx->stream, hipStreamNonBlocking, 0));
    ctx->orb.init(cfg->orb_nfeatures, cfg->orb_scale_factor, cfg->orb_nlevels,
                  cfg->orb_ini_th_fast, cfg->orb_min_th_fast);
    ctx->engine.setup(cfg->width, cfg->height, ctx->orb, cfg->max_batch > 0 ? cfg->max_batch : 1);
  } catch (const ArgError& e) {
    g_create_error = e.msg;
    delete ctx;
    return nullptr;
  } catch (const DeviceError& e) {
    g_create_error = e.msg;
    delete ctx;
    return nullptr;
  }
  return ctx;
}

void mmt_destroy(mmt_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->cfg.device_id);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  (void)hipFree(ctx->d_in);
  (void)hipFree(ctx->d_kps);
  (void)hipFree(ctx->d_desc);
  (void)hipFree(ctx->d_n);
  (void)hipFree(ctx->t_bgr);
  (void)hipFree(ctx->t_disp);
  (void)hipFree(ctx->t_flow);
  (void)hipFree(ctx->t_mask);
  (void)hipFree(ctx->s_mask);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

int mmt_orb_levels(const mmt_ctx* ctx, float* scale, float* sigma2, int* n_per_level,
                   int* level_w, int* level_h) {
  if (!ctx) return MMT_EINVAL;
  const auto& lv = ctx->engine.levels();
  for (int l = 0; l < ctx->orb.nlevels; l++) {
    if (scale) scale[l] = ctx->orb.scale[l];
    if (sigma2) sigma2[l] = ctx->orb.sigma2[l];
    if (n_per_level) n_per_level[l] = ctx->orb.nPerLevel[l];
    if (level_w) level_w[l] = lv[l].w;
    if (level_h) level_h[l] = lv[l].h;
  }
  return MMT_OK;
}

int mmt_orb_capacity(const mmt_ctx* ctx) { return ctx ? ctx->engine.capacity() : MMT_EINVAL; }

static void ensure_staging(mmt_ctx* ctx, int nframes) {
  const size_t fb = (size_t)ctx->cfg.width * ctx->cfg.height;
  if (ctx->staged_frames >= nframes) return;
  (void)hipFree(ctx->d_in);
  (void)hipFree(ctx->d_kps);
  (void)hipFree(ctx->d_desc);
  (void)hipFree(ctx->d_n);
  ctx->d_in = nullptr;
  ctx->d_kps = nullptr;
  ctx->d_desc = nullptr;
  ctx->d_n = nullptr;
  const int cap = ctx->engine.capacity();
  MMT_HIP(hipMalloc((void**)&ctx->d_in, fb * nframes));
  MMT_HIP(hipMalloc((void**)&ctx->d_kps, sizeof(mmt_kp) * (size_t)cap * nframes));
  MMT_HIP(hipMalloc((void**)&ctx->d_desc, (size_t)32 * cap * nframes));
  MMT_HIP(hipMalloc((void**)&ctx->d_n, sizeof(int) * nframes));
  ctx->staged_frames = nframes;
}

int mmt_orb_extract_batch(mmt_ctx* ctx, const uint8_t* const* grays, int nframes, int stride,
                          mmt_kp* kps, uint8_t* desc, int cap_per_frame, int* n_per_frame) {
  if (!ctx || !grays || !kps || !desc || !n_per_frame || nframes < 1) return MMT_EINVAL;
  return guard(ctx, [&] {
    const int w = ctx->cfg.width, h = ctx->cfg.height;
    if (stride < w) throw ArgError("stride < width");
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    const int cap = ctx->engine.capacity();
    int done = 0;
    std::vector<int> counts(nframes, 0);
    while (done < nframes) {
      const int nb = std::min(nframes - done, ctx->cfg.max_batch > 0 ? ctx->cfg.max_batch : 1);
      ensure_staging(ctx, nb);
      const size_t fb = (size_t)w * h;
      for (int f = 0; f < nb; f++)
        MMT_HIP(hipMemcpy2DAsync(ctx->d_in + fb * f, w, grays[done + f], stride, w, h,
                                 hipMemcpyHostToDevice, ctx->stream));
      ctx->engine.run(ctx->d_in, nb, fb, ctx->d_kps, ctx->d_desc, cap, ctx->d_n, ctx->stream);
      MMT_HIP(hipMemcpyAsync(counts.data() + done, ctx->d_n, sizeof(int) * nb,
                             hipMemcpyDeviceToHost, ctx->stream));
      ctx->engine.check_flags(ctx->stream);  // synchronises the stream
      for (int f = 0; f < nb; f++) {
        const int n = counts[done + f];
        n_per_frame[done + f] = n;
        if (n > cap_per_frame) throw ArgError("cap_per_frame too small");
        MMT_HIP(hipMemcpyAsync(kps + (size_t)(done + f) * cap_per_frame,
                               ctx->d_kps + (size_t)f * cap, sizeof(mmt_kp) * n,
                               hipMemcpyDeviceToHost, ctx->stream));
        MMT_HIP(hipMemcpyAsync(desc + (size_t)(done + f) * cap_per_frame * 32,
                               ctx->d_desc + (size_t)f * cap * 32, (size_t)32 * n,
                               hipMemcpyDeviceToHost, ctx->stream));
      }
      MMT_HIP(hipStreamSynchronize(ctx->stream));
      done += nb;
    }
  });
}

int mmt_orb_extract(mmt_ctx* ctx, const uint8_t* gray, int w, int h, int stride, mmt_kp* kps,
                    uint8_t* desc, int cap, int* n) {
  if (!ctx || !gray || !kps || !desc || !n) return MMT_EINVAL;
  if (w != ctx->cfg.width || h != ctx->cfg.height) {
    ctx->err = "image size differs from the context configuration";
    return MMT_EINVAL;
  }
  const int fcap = ctx->engine.capacity();
  std::vector<mmt_kp> tk;
  std::vector<uint8_t> td;
  try {
    tk.resize(fcap);
    td.resize((size_t)fcap * 32);
  } catch (const std::bad_alloc&) {
    return MMT_ENOMEM;
  }
  const uint8_t* frames[1] = {gray};
  int cnt = 0;
  const int rc = mmt_orb_extract_batch(ctx, frames, 1, stride, tk.data(), td.data(), fcap, &cnt);
  if (rc) return rc;
  *n = cnt;
  if (cnt > cap) {
    ctx->err = "keypoint capacity too small";
    return MMT_ENOSPC;
  }
  memcpy(kps, tk.data(), sizeof(mmt_kp) * cnt);
  memcpy(desc, td.data(), (size_t)32 * cnt);
  return MMT_OK;
}

int mmt_orb_extract_device(mmt_ctx* ctx, const uint8_t* d_gray, int nframes, size_t frame_pitch,
                           mmt_kp* d_kps, uint8_t* d_desc, int cap_per_frame, int* d_n,
                           void* stream) {
  if (!ctx || !d_gray || !d_kps || !d_desc || !d_n) return MMT_EINVAL;
  return guard(ctx, [&] {
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    ctx->engine.run(d_gray, nframes, frame_pitch, d_kps, d_desc, cap_per_frame, d_n, s);
  });
}

int mmt_orb_device_status(mmt_ctx* ctx, void* stream) {
  if (!ctx) return MMT_EINVAL;
  return guard(ctx, [&] {
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    ctx->engine.check_flags(stream ? (hipStream_t)stream : ctx->stream);
  });
}

int mmt_debug_orb_raise(mmt_ctx* ctx, int flags) {
  if (!ctx) return MMT_EINVAL;
  return guard(ctx, [&] {
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    ctx->engine.raise_flags(flags, ctx->stream);
  });
}

// ---- stereo frames (Frame.cc:79-159, 849-1038) -------------------------------------------------
static mmt::StereoLevels stereo_levels(const mmt_ctx* ctx) {
  mmt::StereoLevels lv;
  memset(&lv, 0, sizeof(lv));
  const auto& L = ctx->engine.levels();
  lv.nlevels = ctx->orb.nlevels;
  lv.rows = ctx->cfg.height;
  lv.cols = ctx->cfg.width;
  for (int l = 0; l < lv.nlevels; l++) {
    lv.w[l] = L[l].w;
    lv.h[l] = L[l].h;
    lv.off[l] = L[l].off;
    lv.scale[l] = ctx->orb.scale[l];
    lv.invScale[l] = ctx->orb.invScale[l];
  }
  return lv;
}

static void check_stereo_common(mmt_ctx* ctx, const char* who, int w, int h, int stride) {
  if (w != ctx->cfg.width || h != ctx->cfg.height)
    throw ArgError("image size differs from the context configuration");
  if (stride < w) throw ArgError("stride < width");
  if (ctx->cfg.max_batch < 2)
    throw ArgError(std::string(who) + " needs config.max_batch >= 2: the device pyramid is "
                   "frame-major per batch slot and a stereo pair takes two slots");
  if (ctx->orb.nlevels > mmt::kStereoMaxLevels) throw ArgError("too many pyramid levels");
}

// The keys Frame::ComputeStereoMatches would index out of bounds with (pin (c) of mmt_stereo.hip),
// tested with the float operations of the kernels.
static void check_stereo_keys(const mmt::StereoLevels& lv, int nl, const mmt_kp* kl, int nr,
                              const mmt_kp* kr) {
  for (int i = 0; i < nl; i++) {
    const mmt_kp& k = kl[i];
    if (k.octave < 0 || k.octave >= lv.nlevels)
      throw ArgError("left key " + std::to_string(i) + ": octave outside the pyramid");
    const float s = lv.invScale[k.octave];
    const float u = roundf(k.x * s), v = roundf(k.y * s);
    if (!(u - 5.f >= 0.f && u + 5.f < (float)lv.w[k.octave] && v - 5.f >= 0.f &&
          v + 5.f < (float)lv.h[k.octave] && k.y >= 0.f && k.y < (float)lv.rows))
      throw ArgError("left key " + std::to_string(i) + ": its 11 x 11 window leaves its level");
  }
  for (int i = 0; i < nr; i++) {
    const mmt_kp& k = kr[i];
    if (k.octave < 0 || k.octave >= lv.nlevels)
      throw ArgError("right key " + std::to_string(i) + ": octave outside the pyramid");
    const float r = 1.2f * lv.scale[k.octave];
    const float top = k.y + r, bot = k.y - r;
    if (!(floorf(bot) >= 0.f && ceilf(top) < (float)lv.rows))
      throw ArgError("right key " + std::to_string(i) + ": its row range leaves the image");
  }
}

static void stage_pair(mmt_ctx* ctx, const uint8_t* left, const uint8_t* right, int stride) {
  const int w = ctx->cfg.width, h = ctx->cfg.height;
  ensure_staging(ctx, 2);
  const size_t fb = (size_t)w * h;
  MMT_HIP(hipMemcpy2DAsync(ctx->d_in, w, left, stride, w, h, hipMemcpyHostToDevice, ctx->stream));
  MMT_HIP(hipMemcpy2DAsync(ctx->d_in + fb, w, right, stride, w, h, hipMemcpyHostToDevice,
                           ctx->stream));
}

int mmt_stereo_matches(mmt_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h,
                       int stride, int n_left, const mmt_kp* kps_left, const uint8_t* desc_left,
                       int n_right, const mmt_kp* kps_right, const uint8_t* desc_right, float* uR,
                       float* depth, int32_t* right_idx, int32_t* best_dist, int32_t* sad,
                       mmt_stereo_counters* counters) {
  if (!ctx || !left || !right || !uR || !depth || !right_idx || !counters) return MMT_EINVAL;
  return guard(ctx, [&] {
    check_stereo_common(ctx, "mmt_stereo_matches", w, h, stride);
    if (n_left < 0 || n_left > mmt::kMaxMatchKeys || n_right < 0 || n_right > mmt::kMaxMatchKeys)
      throw ArgError("key count outside [0, 16384]");
    if ((n_left > 0 && (!kps_left || !desc_left)) || (n_right > 0 && (!kps_right || !desc_right)))
      throw ArgError("null key arrays");
    const mmt::StereoLevels lv = stereo_levels(ctx);
    check_stereo_keys(lv, n_left, kps_left, n_right, kps_right);
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    hipStream_t s = ctx->stream;
    stage_pair(ctx, left, right, stride);
    ctx->engine.build_pyramids(ctx->d_in, 2, (size_t)w * h, s);
    DevBuf<mmt_kp> kl(n_left), kr(n_right);
    DevBuf<uint8_t> dl((size_t)32 * n_left), dr((size_t)32 * n_right);
    DevBuf<int> dn(2);
    const int ns[2] = {n_left, n_right};
    dn.up(ns, 2, s);
    kl.up(kps_left, n_left, s);
    dl.up(desc_left, (size_t)32 * n_left, s);
    kr.up(kps_right, n_right, s);
    dr.up(desc_right, (size_t)32 * n_right, s);
    mmt::StereoMatcher& M = ctx->stereo;
    M.ensure(h, std::max(std::max(n_left, n_right), 1), ctx->orb.scale[ctx->orb.nlevels - 1]);
    const mmt::StereoSide L{ctx->engine.pyramid(), kl.p, dl.p, dn.p};
    const mmt::StereoSide R{ctx->engine.pyramid() + ctx->engine.pyramid_stride(), kr.p, dr.p,
                            dn.p + 1};
    M.run(lv, L, R, n_left, n_right, ctx->cfg.bf, s);
    if (n_left > 0) {
      const size_t nb = sizeof(float) * (size_t)n_left;
      MMT_HIP(hipMemcpyAsync(uR, M.uR, nb, hipMemcpyDeviceToHost, s));
      MMT_HIP(hipMemcpyAsync(depth, M.depth, nb, hipMemcpyDeviceToHost, s));
      MMT_HIP(hipMemcpyAsync(right_idx, M.right_idx, nb, hipMemcpyDeviceToHost, s));
      if (best_dist) MMT_HIP(hipMemcpyAsync(best_dist, M.best_dist, nb, hipMemcpyDeviceToHost, s));
      if (sad) MMT_HIP(hipMemcpyAsync(sad, M.sad, nb, hipMemcpyDeviceToHost, s));
    }
    MMT_HIP(hipMemcpyAsync(counters, M.counters, sizeof(*counters), hipMemcpyDeviceToHost, s));
    MMT_HIP(hipStreamSynchronize(s));
  });
}

int mmt_stereo_frame(mmt_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h,
                     int stride, const int32_t* mask, mmt_kp* kps, uint8_t* desc, int cap, int* n,
                     mmt_kp* kps_right, uint8_t* desc_right, int cap_right, int* n_right,
                     float* uR, float* depth, int32_t* right_idx, int32_t* sem_label,
                     mmt_stereo_counters* counters) {
  if (!ctx || !left || !right || !kps || !desc || !n || !kps_right || !desc_right || !n_right ||
      !uR || !depth || !right_idx || !counters || (mask && !sem_label))
    return MMT_EINVAL;
  bool short_cap = false;
  const int rc = guard(ctx, [&] {
    check_stereo_common(ctx, "mmt_stereo_frame", w, h, stride);
    if (cap < 0 || cap_right < 0) throw ArgError("negative capacity");
    const int ecap = ctx->engine.capacity();
    if (ecap > mmt::kMaxMatchKeys)
      throw ArgError("mmt_orb_capacity() above 16384 keys: too many for the stereo matcher");
    const mmt::StereoLevels lv = stereo_levels(ctx);
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    hipStream_t s = ctx->stream;
    const size_t fb = (size_t)w * h;
    mmt::StereoMatcher& M = ctx->stereo;
    M.ensure(h, ecap, ctx->orb.scale[ctx->orb.nlevels - 1]);
    if (mask && !ctx->s_mask) MMT_HIP(hipMalloc((void**)&ctx->s_mask, fb * sizeof(int32_t)));
    stage_pair(ctx, left, right, stride);
    if (mask)
      MMT_HIP(hipMemcpyAsync(ctx->s_mask, mask, fb * sizeof(int32_t), hipMemcpyHostToDevice, s));
    // extraction, matching and the median stage back to back on the stream
    ctx->engine.run(ctx->d_in, 2, fb, ctx->d_kps, ctx->d_desc, ecap, ctx->d_n, s);
    const mmt::StereoSide L{ctx->engine.pyramid(), ctx->d_kps, ctx->d_desc, ctx->d_n};
    const mmt::StereoSide R{ctx->engine.pyramid() + ctx->engine.pyramid_stride(),
                            ctx->d_kps + ecap, ctx->d_desc + (size_t)32 * ecap, ctx->d_n + 1};
    M.run(lv, L, R, ecap, ecap, ctx->cfg.bf, s);
    if (mask) M.sem_labels(L, ecap, ctx->s_mask, w, h, s);
    int counts[2] = {0, 0};
    MMT_HIP(hipMemcpyAsync(counts, ctx->d_n, sizeof(counts), hipMemcpyDeviceToHost, s));
    ctx->engine.check_flags(s);  // synchronises the stream
    *n = counts[0];
    *n_right = counts[1];
    if (counts[0] > cap || counts[1] > cap_right) {
      short_cap = true;
      return;
    }
    const size_t nl = (size_t)counts[0], nr = (size_t)counts[1];
    if (nl > 0) {
      MMT_HIP(hipMemcpyAsync(kps, L.kps, sizeof(mmt_kp) * nl, hipMemcpyDeviceToHost, s));
      MMT_HIP(hipMemcpyAsync(desc, L.desc, 32 * nl, hipMemcpyDeviceToHost, s));
      MMT_HIP(hipMemcpyAsync(uR, M.uR, 4 * nl, hipMemcpyDeviceToHost, s));
      MMT_HIP(hipMemcpyAsync(depth, M.depth, 4 * nl, hipMemcpyDeviceToHost, s));
      MMT_HIP(hipMemcpyAsync(right_idx, M.right_idx, 4 * nl, hipMemcpyDeviceToHost, s));
      if (mask) MMT_HIP(hipMemcpyAsync(sem_label, M.sem, 4 * nl, hipMemcpyDeviceToHost, s));
    }
    if (nr > 0) {
      MMT_HIP(hipMemcpyAsync(kps_right, R.kps, sizeof(mmt_kp) * nr, hipMemcpyDeviceToHost, s));
      MMT_HIP(hipMemcpyAsync(desc_right, R.desc, 32 * nr, hipMemcpyDeviceToHost, s));
    }
    MMT_HIP(hipMemcpyAsync(counters, M.counters, sizeof(*counters), hipMemcpyDeviceToHost, s));
    MMT_HIP(hipStreamSynchronize(s));
  });
  if (rc == MMT_OK && short_cap) {
    ctx->err = "keypoint capacity too small";
    return MMT_ENOSPC;
  }
  return rc;
}

static void ensure_tracker(mmt_ctx* ctx) {
  if (ctx->tracker_ready) return;
  const int B = ctx->cfg.max_batch > 0 ? ctx->cfg.max_batch : 1;
  ctx->tracker.setup(ctx->cfg, &ctx->engine, B);
  ctx->tracker_ready = true;
}

static void fill_results(const std::vector<mmt::FrameOut>& outs, mmt_frame_result* res,
                         mmt_motion* objs, int objs_cap) {
  for (size_t f = 0; f < outs.size(); f++) {
    const mmt::FrameOut& o = outs[f];
    mmt_frame_result& r = res[f];
    memcpy(r.Tcw, o.Tcw, sizeof(r.Tcw));
    r.initialized = o.initialized;
    r.n_keypoints = o.n_keys;
    r.n_obj_samples = o.n_obj_samples;
    r.ego_iterations = o.ego_iterations;
    r.ego_inliers = o.ego_inliers;
    r.n_objects = (int)o.objects.size();
    r.map_state = o.map.state;
    r.map_matches_mm = o.map.matches_mm;
    r.map_inliers_local = o.map.inliers_local;
    r.n_keyframes = o.map.n_keyframes;
    r.n_mappoints = o.map.n_mappoints;
    r.new_keyframe = o.map.new_keyframe;
    memcpy(r.Tcw_map, o.map.Tcw_map, sizeof(r.Tcw_map));
    r.frame_index = (int32_t)o.seq;
    r.objects_frame = (int32_t)o.obj_seq;
    if (!objs) continue;
    for (int i = 0; i < (int)o.objects.size() && i < objs_cap; i++) {
      const mmt::ObjOut& s = o.objects[i];
      mmt_motion& m = objs[f * objs_cap + i];
      m.label = s.label;
      m.sem_label = s.sem_label;
      m.n_points = s.n_points;
      m.n_inliers = s.n_inliers;
      m.n_ransac_inliers = s.n_ransac_inliers;
      m.n_mm_inliers = s.n_mm_inliers;
      m.n_solve = s.n_solve;
      m.iterations = s.iterations;
      memcpy(m.world_motion, s.motion, 64);
      memcpy(m.cam_pose, s.X, 64);
      memcpy(m.init_pose, s.init, 64);
      memcpy(m.centre_pre, s.centre_pre, 12);
    }
  }
}

int mmt_profile_enable(mmt_ctx* ctx, int on) {
  if (!ctx) return MMT_EINVAL;
  return guard(ctx, [&] {
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    ensure_tracker(ctx);
    ctx->tracker.set_profiling(on != 0);
  });
}

int mmt_profile_read(mmt_ctx* ctx, mmt_profile* out, int reset) {
  if (!ctx || !out) return MMT_EINVAL;
  return guard(ctx, [&] {
    ensure_tracker(ctx);
    long long l = 0, f = 0;
    ctx->tracker.read_profile(&out->orb_ms, &l, &f, reset != 0);
    out->orb_launches = l;
    out->orb_frames = f;
  });
}

int mmt_reset(mmt_ctx* ctx) {
  if (!ctx) return MMT_EINVAL;
  return guard(ctx, [&] {
    ensure_tracker(ctx);
    ctx->tracker.reset();
    ctx->flushed.clear();
  });
}

int mmt_set_deferred_objects(mmt_ctx* ctx, int on) {
  if (!ctx) return MMT_EINVAL;
  return guard(ctx, [&] {
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    ensure_tracker(ctx);
    ctx->tracker.set_deferred(on != 0);
    if (!on) ctx->flushed.clear();
  });
}

int mmt_flush_objects(mmt_ctx* ctx, mmt_frame_result* res, mmt_motion* objs, int objs_cap,
                      int res_cap, int* n) {
  if (!ctx || !res || !n || res_cap < 1 || objs_cap < 0) return MMT_EINVAL;
  *n = 0;
  return guard(ctx, [&] {
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    ensure_tracker(ctx);
    if (ctx->flushed.empty()) {
      std::vector<mmt::FrameOut> outs;
      ctx->tracker.flush_deferred(outs);
      for (auto& o : outs) ctx->flushed.push_back(std::move(o));
    }
    std::vector<mmt::FrameOut> part;
    while (!ctx->flushed.empty() && (int)part.size() < res_cap) {
      part.push_back(std::move(ctx->flushed.front()));
      ctx->flushed.pop_front();
    }
    for (auto& o : part) o.seq = -1;  // flush records carry objects only
    memset(res, 0, sizeof(mmt_frame_result) * (size_t)part.size());
    fill_results(part, res, objs, objs_cap);
    *n = (int)part.size();
  });
}

// Records a partial mmt_flush_objects left for a later call: tracking more frames before they
// are drained would deliver newer frames' motions ahead of them (the header promises order).
static int flush_owed(mmt_ctx* ctx) {
  if (ctx->flushed.empty()) return 0;
  ctx->err = "mmt_flush_objects has undelivered records: drain it before tracking more frames";
  return MMT_ESTATE;
}

int mmt_track_rgbd_chunk_device(mmt_ctx* ctx, int nframes, const uint8_t* d_bgr,
                                size_t bgr_pitch, const uint16_t* d_disp, size_t disp_pitch,
                                const float* d_flow, size_t flow_pitch, const int32_t* d_mask,
                                size_t mask_pitch, mmt_frame_result* res, mmt_motion* objs,
                                int objs_cap, void* stream) {
  if (!ctx || !d_bgr || !d_disp || !d_flow || !d_mask || !res || nframes < 1) return MMT_EINVAL;
  if (const int rc = flush_owed(ctx)) return rc;
  return guard(ctx, [&] {
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    ensure_tracker(ctx);
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    std::vector<mmt::FrameOut> outs;
    ctx->tracker.track_chunk(d_bgr, bgr_pitch, d_disp, disp_pitch, d_flow, flow_pitch, d_mask,
                             mask_pitch, nframes, outs, s);
    fill_results(outs, res, objs, objs_cap);
  });
}

// device staging of the host-buffer entry points, nframes frames (frame-major, tight pitches)
static void ensure_track_staging(mmt_ctx* ctx, int nframes) {
  if (ctx->t_frames >= nframes) return;
  const size_t npix = (size_t)ctx->cfg.width * ctx->cfg.height;
  (void)hipFree(ctx->t_bgr);
  (void)hipFree(ctx->t_disp);
  (void)hipFree(ctx->t_flow);
  (void)hipFree(ctx->t_mask);
  ctx->t_bgr = nullptr;
  ctx->t_disp = nullptr;
  ctx->t_flow = nullptr;
  ctx->t_mask = nullptr;
  ctx->t_frames = 0;
  MMT_HIP(hipMalloc((void**)&ctx->t_bgr, npix * 3 * nframes));
  MMT_HIP(hipMalloc((void**)&ctx->t_disp, npix * 2 * nframes));
  MMT_HIP(hipMalloc((void**)&ctx->t_flow, npix * 8 * nframes));
  MMT_HIP(hipMalloc((void**)&ctx->t_mask, npix * 4 * nframes));
  ctx->t_frames = nframes;
}

static void track_host_frames(mmt_ctx* ctx, int nframes, const uint8_t* const* bgr,
                              const uint16_t* const* disp, const float* const* flow,
                              const int32_t* const* mask, mmt_frame_result* res, mmt_motion* objs,
                              int objs_cap) {
  MMT_HIP(hipSetDevice(ctx->cfg.device_id));
  ensure_tracker(ctx);
  ensure_track_staging(ctx, nframes);
  const size_t npix = (size_t)ctx->cfg.width * ctx->cfg.height;
  hipStream_t s = ctx->stream;
  for (int f = 0; f < nframes; f++) {
    MMT_HIP(hipMemcpyAsync(ctx->t_bgr + npix * 3 * f, bgr[f], npix * 3, hipMemcpyHostToDevice, s));
    MMT_HIP(hipMemcpyAsync(ctx->t_disp + npix * f, disp[f], npix * 2, hipMemcpyHostToDevice, s));
    MMT_HIP(hipMemcpyAsync(ctx->t_flow + npix * 2 * f, flow[f], npix * 8, hipMemcpyHostToDevice, s));
    MMT_HIP(hipMemcpyAsync(ctx->t_mask + npix * f, mask[f], npix * 4, hipMemcpyHostToDevice, s));
  }
  std::vector<mmt::FrameOut> outs;
  ctx->tracker.track_chunk(ctx->t_bgr, npix * 3, ctx->t_disp, npix * 2, ctx->t_flow, npix * 8,
                           ctx->t_mask, npix * 4, nframes, outs, s);
  fill_results(outs, res, objs, objs_cap);
}

int mmt_track_rgbd(mmt_ctx* ctx, const uint8_t* bgr, const uint16_t* disp256,
                   const float* flow_uv, const int32_t* mask, double timestamp,
                   mmt_frame_result* res, mmt_motion* objs, int objs_cap) {
  (void)timestamp;
  if (!ctx || !bgr || !disp256 || !flow_uv || !mask || !res) return MMT_EINVAL;
  if (const int rc = flush_owed(ctx)) return rc;
  return guard(ctx, [&] {
    track_host_frames(ctx, 1, &bgr, &disp256, &flow_uv, &mask, res, objs, objs_cap);
  });
}

int mmt_track_rgbd_chunk(mmt_ctx* ctx, int nframes, const uint8_t* const* bgr,
                         const uint16_t* const* disp256, const float* const* flow_uv,
                         const int32_t* const* mask, mmt_frame_result* res, mmt_motion* objs,
                         int objs_cap) {
  if (!ctx || !bgr || !disp256 || !flow_uv || !mask || !res || nframes < 1) return MMT_EINVAL;
  for (int f = 0; f < nframes; f++)
    if (!bgr[f] || !disp256[f] || !flow_uv[f] || !mask[f]) return MMT_EINVAL;
  if (const int rc = flush_owed(ctx)) return rc;
  return guard(ctx, [&] {
    if (nframes > std::max(1, ctx->cfg.max_batch))
      throw ArgError("chunk larger than config.max_batch");
    track_host_frames(ctx, nframes, bgr, disp256, flow_uv, mask, res, objs, objs_cap);
  });
}

void* mmt_host_alloc(mmt_ctx* ctx, size_t bytes) {
  if (!ctx || bytes == 0) return nullptr;
  void* p = nullptr;
  if (hipSetDevice(ctx->cfg.device_id) != hipSuccess) return nullptr;
  if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
  return p;
}

void mmt_host_free(mmt_ctx* ctx, void* p) {
  (void)ctx;
  if (p) (void)hipHostFree(p);
}

int mmt_frame_samples(mmt_ctx* ctx, float* static_xy, int static_cap, int* n_static,
                      float* obj_xy, int32_t* obj_label, int obj_cap, int* n_obj) {
  if (!ctx || !n_static || !n_obj || static_cap < 0 || obj_cap < 0) return MMT_EINVAL;
  return guard(ctx, [&] {
    *n_static = *n_obj = 0;
    if (!ctx->tracker_ready) return;
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    ctx->tracker.frame_samples(static_xy, static_cap, n_static, obj_xy, obj_label, obj_cap, n_obj,
                               ctx->stream);
  });
}

int mmt_map_counters_read(mmt_ctx* ctx, mmt_map_counters* out) {
  if (!ctx || !out) return MMT_EINVAL;
  return guard(ctx, [&] {
    memset(out, 0, sizeof(*out));
    if (!ctx->tracker_ready) return;
    const mmt::MappingStats& m = ctx->tracker.mapping_stats();
    out->n_ba = m.n_ba;
    out->n_fused = m.n_fused;
    out->n_culled = m.n_culled;
    out->n_ba_erased = m.n_ba_erased;
    out->ba_trials = m.ba_trials;
    out->ba_edges = m.ba_edges;
    out->ba_kfs = m.ba_kfs;
    out->ba_pts = m.ba_pts;
    out->ba_max_opt = m.ba_max_opt;
    out->fuse_launches = m.fuse_launches;
    out->fuse_queries = m.fuse_queries;
    out->fuse_relaunches = m.fuse_relaunches;
    out->lm_us = m.lm_us;
    out->ba_us = m.ba_us;
    out->fuse_us = m.fuse_us;
    out->d2_split_fallbacks = ctx->tracker.split_fallbacks();
    out->n_reparent = m.n_reparent;
  });
}

int mmt_set_keyframe_culling_ratio(mmt_ctx* ctx, double ratio) {
  if (!ctx || !(ratio >= 0)) return MMT_EINVAL;
  return guard(ctx, [&] {
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    ensure_tracker(ctx);
    ctx->tracker.set_cull_ratio(ratio);
  });
}

int mmt_load_vocabulary(mmt_ctx* ctx, const char* path) {
  if (!ctx || !path) return MMT_EINVAL;
  bool late = false;
  const int rc = guard(ctx, [&] {
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    ensure_tracker(ctx);
    if (ctx->tracker.map().n_keyframes() > 0 || ctx->tracker.map().state() != 0) {
      late = true;
      return;
    }
    std::unique_ptr<mmt::Vocabulary> v(new mmt::Vocabulary());
    v->load_text(path);
    ctx->tracker.set_vocabulary(v.get());
    ctx->voc = std::move(v);
  });
  if (rc == MMT_OK && late) {
    ctx->err = "mmt_load_vocabulary: load the vocabulary before the first frame";
    return MMT_ESTATE;
  }
  return rc;
}

int mmt_train_vocabulary(mmt_ctx* ctx, const uint8_t* desc, const int32_t* image_start,
                         int n_images, const mmt_voc_train_params* params,
                         mmt_voc_train_stats* stats) {
  if (!ctx || !desc || !image_start || n_images <= 0 || !params || !stats) return MMT_EINVAL;
  bool late = false;
  const int rc = guard(ctx, [&] {
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    ensure_tracker(ctx);
    if (ctx->tracker.map().n_keyframes() > 0 || ctx->tracker.map().state() != 0) {
      late = true;
      return;
    }
    std::unique_ptr<mmt::Vocabulary> v(new mmt::Vocabulary());
    mmt::train_vocabulary(desc, image_start, n_images, *params, *v, *stats, ctx->stream);
    ctx->tracker.set_vocabulary(v.get());
    ctx->voc = std::move(v);
  });
  if (rc == MMT_OK && late) {
    ctx->err = "mmt_train_vocabulary: train the vocabulary before the first frame";
    return MMT_ESTATE;
  }
  return rc;
}

int mmt_save_vocabulary(mmt_ctx* ctx, const char* path) {
  if (!ctx || !path) return MMT_EINVAL;
  return guard(ctx, [&] {
    if (!ctx->voc) throw mmt::ArgError("mmt_save_vocabulary: no vocabulary loaded or trained");
    ctx->voc->save_text(path);
  });
}

int mmt_bow_counters_read(mmt_ctx* ctx, mmt_bow_counters* out) {
  if (!ctx || !out) return MMT_EINVAL;
  return guard(ctx, [&] {
    memset(out, 0, sizeof(*out));
    if (!ctx->tracker_ready) return;
    const mmt::BowStatsH& b = ctx->tracker.bow_stats();
    out->bow_frames = b.n_bow_frames;
    out->trk = b.n_trk;
    out->trk_ok = b.n_trk_ok;
    out->reloc = b.n_reloc;
    out->reloc_ok = b.n_reloc_ok;
    out->reloc_cands = b.n_reloc_cands;
    out->pnp_found = b.n_pnp_found;
    out->sbp_rounds = b.n_sbp_rounds;
    out->triangulated = b.n_triangulated;
    out->sft_matches = b.n_sft_matches;
    out->kfdb = b.n_kfdb;
  });
}

int mmt_map_dump(mmt_ctx* ctx, int32_t* sizes, const mmt_map_dump_arrays* out) {
  if (!ctx || !sizes) return MMT_EINVAL;
  return guard(ctx, [&] {
    if (!ctx->tracker_ready) {
      memset(sizes, 0, 7 * sizeof(int32_t));
      return;
    }
    ctx->tracker.map().dump(sizes, out);
  });
}

// ---- loop detection (LoopClosing::DetectLoop, KeyFrameDatabase; mmt_loop.hip, mmt_loopdetect.cpp)
int mmt_loop_reset(mmt_ctx* ctx, int scoring) {
  if (!ctx) return MMT_EINVAL;
  return guard(ctx, [&] {
    if (scoring != 0 && scoring != 1) throw ArgError("mmt_loop_reset: scoring is 0 (L1) or 1 (L2)");
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    MMT_HIP(hipStreamSynchronize(ctx->stream));
    ctx->loop.reset();
    ctx->loopdet.reset(scoring);
  });
}

int mmt_loop_set_bow(mmt_ctx* ctx, int32_t kf_id, const mmt_bow_vector* v) {
  if (!ctx || !v) return MMT_EINVAL;
  return guard(ctx, [&] {
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    ctx->loop.set_bow(kf_id, *v, ctx->stream);
  });
}

int mmt_loop_db_add(mmt_ctx* ctx, int32_t kf_id) {
  if (!ctx) return MMT_EINVAL;
  return guard(ctx, [&] {
    if (ctx->loop.table.find(kf_id) < 0) throw ArgError("mmt_loop_db_add: unknown keyframe id");
    if (!ctx->loop.table.db_add(kf_id))
      throw ArgError("mmt_loop_db_add: the keyframe is in the database already");
  });
}

int mmt_loop_db_erase(mmt_ctx* ctx, int32_t kf_id) {
  if (!ctx) return MMT_EINVAL;
  return guard(ctx, [&] {
    if (!ctx->loop.table.db_erase(kf_id)) throw ArgError("mmt_loop_db_erase: unknown keyframe id");
  });
}

static void copy_ids(const std::vector<int32_t>& v, int32_t* out, int cap, const char* what) {
  if ((int)v.size() > cap || (!v.empty() && !out))
    throw ArgError(std::string(what) + ": output buffer too small");
  if (!v.empty()) memcpy(out, v.data(), sizeof(int32_t) * v.size());
}

int mmt_detect_loop_candidates(mmt_ctx* ctx, int32_t kf_id, float min_score,
                               const mmt_covis_graph* graph, int32_t* cand_out, int cap,
                               int* n_out) {
  if (!ctx || !graph || !n_out || cap < 0) return MMT_EINVAL;
  return guard(ctx, [&] {
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    if (kf_id < 0 || kf_id >= graph->n_kf)
      throw ArgError("mmt_detect_loop_candidates: keyframe id outside the graph");
    const std::vector<mmt::LoopScore>& sc =
        ctx->loop.score(kf_id, ctx->loopdet.scoring(), ctx->stream);
    std::vector<int32_t> cand;
    if (!ctx->loopdet.candidates(ctx->loop.table, sc.data(), kf_id, min_score, *graph, cand))
      throw ArgError("mmt_detect_loop_candidates: " + ctx->loopdet.error());
    *n_out = (int)cand.size();
    copy_ids(cand, cand_out, cap, "mmt_detect_loop_candidates");
  });
}

int mmt_detect_loop(mmt_ctx* ctx, int32_t kf_id, int32_t last_loop_kf_id, int consistency_th,
                    const mmt_covis_graph* graph, mmt_loop_result* result, int32_t* cand_out,
                    int32_t* enough_out, int cap) {
  if (!ctx || !graph || !result || cap < 0) return MMT_EINVAL;
  return guard(ctx, [&] {
    MMT_HIP(hipSetDevice(ctx->cfg.device_id));
    mmt::LoopSlotTable& T = ctx->loop.table;
    const int slot = T.find(kf_id);
    if (slot < 0) throw ArgError("mmt_detect_loop: unknown keyframe id");
    if (T.slots[slot].member) throw ArgError("mmt_detect_loop: the keyframe is in the database");
    const bool early = mmt::LoopDetector::early_exit(kf_id, last_loop_kf_id);
    if (!early && (kf_id < 0 || kf_id >= graph->n_kf))
      throw ArgError("mmt_detect_loop: keyframe id outside the graph");
    const mmt::LoopScore* sc = nullptr;
    if (!early) sc = ctx->loop.score(kf_id, ctx->loopdet.scoring(), ctx->stream).data();
    // detect() refuses more than `cap` candidates before it changes the database or the groups
    std::vector<int32_t> cand, enough;
    if (!ctx->loopdet.detect(T, sc, kf_id, last_loop_kf_id, consistency_th, *graph,
                             (cand_out && enough_out) ? cap : 0, *result, cand, enough))
      throw ArgError("mmt_detect_loop: " + ctx->loopdet.error());
    copy_ids(cand, cand_out, cap, "mmt_detect_loop");
    copy_ids(enough, enough_out, cap, "mmt_detect_loop");
  });
}

int mmt_loop_groups_read(mmt_ctx* ctx, int32_t* group_start, int32_t* members, int32_t* counters,
                         int cap_groups, int cap_members, int* n_groups, int* n_members) {
  if (!ctx || !n_groups || !n_members || cap_groups < 0 || cap_members < 0) return MMT_EINVAL;
  return guard(ctx, [&] {
    const auto& G = ctx->loopdet.groups();
    size_t nm = 0;
    for (const auto& g : G) nm += g.first.size();
    *n_groups = (int)G.size();
    *n_members = (int)nm;
    if ((int)G.size() > cap_groups || nm > (size_t)cap_members)
      throw ArgError("mmt_loop_groups_read: output buffer too small");
    if (!group_start || (!G.empty() && !counters) || (nm > 0 && !members))
      throw ArgError("mmt_loop_groups_read: null output arrays");
    int32_t at = 0;
    for (size_t i = 0; i < G.size(); i++) {
      group_start[i] = at;
      counters[i] = G[i].second;
      for (int32_t m : G[i].first) members[at++] = m;
    }
    group_start[G.size()] = at;
  });
}

int mmt_loop_stats(mmt_ctx* ctx, mmt_loop_store_stats* out) {
  if (!ctx || !out) return MMT_EINVAL;
  return guard(ctx, [&] { ctx->loop.stats(*out); });
}

long mmt_debug_fetch(mmt_ctx* ctx, int what, int frame, void* out, size_t cap) {
  if (!ctx || !out) return MMT_EINVAL;
  long r = 0;
  const int rc = guard(ctx, [&] { r = ctx->engine.debug_fetch(what, frame, out, cap, ctx->stream); });
  return rc ? rc : r;
}

}  // extern "C"
