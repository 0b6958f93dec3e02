// multimot_track_amd/csrc/mmt_ctx.h -- the opaque mmt_ctx behind include/mmt.h.
#pragma once
#include <deque>
#include <memory>
#include <new>

#include "mmt_ba.h"
#include "mmt_bow.h"
#include "mmt_internal.h"
#include "mmt_loop.h"
#include "mmt_stereo.h"
#include "mmt_tracker.h"

struct mmt_ctx {
  mmt_config cfg;
  mmt::OrbTables orb;
  mmt::OrbEngine engine;
  hipStream_t stream = nullptr;
  std::string err;
  // staging for the host-pointer entry points
  uint8_t* d_in = nullptr;
  size_t d_in_bytes = 0;
  mmt_kp* d_kps = nullptr;
  uint8_t* d_desc = nullptr;
  int* d_n = nullptr;
  int staged_frames = 0;
  mmt::StereoMatcher stereo;    // mmt_stereo_matches / mmt_stereo_frame (workspace kept across calls)
  int32_t* s_mask = nullptr;    // mmt_stereo_frame's semantic mask on the device
  // tracking (one sequence per context)
  mmt::Tracker tracker;
  bool tracker_ready = false;
  mmt::BARunner ba;  // mmt_local_bundle_adjustment's buffers (kept across calls)
  uint8_t* t_bgr = nullptr;
  uint16_t* t_disp = nullptr;
  float* t_flow = nullptr;
  int32_t* t_mask = nullptr;
  int t_frames = 0;  // frames the t_* staging buffers hold
  std::deque<mmt::FrameOut> flushed;  // mmt_flush_objects records not yet handed out
  std::unique_ptr<mmt::Vocabulary> voc;  // mmt_load_vocabulary (System's ORB vocabulary)
  mmt::LoopStore loop;        // mmt_loop_*: the keyframes' BoW vectors on the device, the database
  mmt::LoopDetector loopdet;  // mmt_detect_loop: mvConsistentGroups
};

// Every C-ABI entry point runs its body through this: internal exceptions become an errno-style
// code and the context's error text; nothing exits.
template <typename F>
inline int guard(mmt_ctx* ctx, F&& body) {
  try {
    body();
  } catch (const mmt::ArgError& e) {
    if (ctx) ctx->err = e.msg;
    return MMT_EINVAL;
  } catch (const mmt::DeviceError& e) {
    if (ctx) ctx->err = e.msg;
    return MMT_EDEVICE;
  } catch (const std::bad_alloc&) {
    if (ctx) ctx->err = "host allocation failed";
    return MMT_ENOMEM;
  }
  return MMT_OK;
}
