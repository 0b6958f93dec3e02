// multimot_track_amd/csrc/mmt_pnp.h -- device record of one object's D5 RANSAC problem.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mmt.h"

namespace mmt {

struct PnPObject {
  // inputs
  const int* n;             // member count (device)
  const int* members;       // ascending sample indices (ObjIdNew[i])
  const float2* last_keys;  // last frame's own object samples (mvObjKeys of mLastFrame)
  const float* last_depth;
  const float2* cur_keys;   // current mvObjKeys (= last mvObjCorres)
  float Tlast[16];
  float fx, fy, cx, cy;
  double reproj, confidence;
  const int* subsets;       // [max_iters][5] RNG((uint64)-1) draws for this count
  int use_mm;               // motion model available (PreObjID != -1)
  float MM[16];             // Tcw * last vObjMod[PreObjID]
  int use_mm_choice;        // set by the host after the counts are known
  // scratch / outputs
  float* pts3;              // [cap][3] pre_3d
  float2* pts2;             // [cap] cur_2d
  double* models;           // [max_iters][6] rvec, tvec
  double* hrec;             // [max_iters][kHypRec] per-hypothesis EPnP state (null space, L, ...)
  double* hout;             // [max_iters][3][kHypOut] err, R, t of the three beta estimates
  int* good;                // [max_iters]
  unsigned long long* masks;  // [max_iters][mask_words]
  int mask_words;
  int* inliers;             // RANSAC inliers (indices into the member list)
  int* mm_inliers;
  int* subset;              // D3 edge -> sample index
  int* n_subset;
  int* result;              // best, maxGood, iterations, n_ransac_inliers, n_mm_inliers,
                            // D6: refined inlier count (6)
  double* Rt;               // R (9), t (3)
  // D6 (PnPsolver) only
  int raw_pixels;           // EPnP inputs are the pixels as they are (add_correspondence)
  int rt_raw;               // refit R without the Rodrigues round trip
  const float* max_err;     // [n] mvMaxError = sigma2 * th2 (CheckInliers thresholds)
  double* hrt;              // [max_iters][12] R, t of each hypothesis' chosen estimate
};

constexpr int kHypRec = 160;  // doubles per hypothesis record
constexpr int kHypOut = 16;   // doubles per (hypothesis, beta variant) result

// RANSAC + refit (the motion-model check is k_obj_stage_b's, mmt_tracker.hip)
void launch_pnp(PnPObject* d_objs, int nobj, int max_iters, hipStream_t st, bool gather = true);
// D6: P4P hypotheses (subsets [K][4]), their chosen estimates (hrt) and CheckInliers (good,
// masks rows 0..K-1)
void launch_p4p_hypotheses(PnPObject* d_obj, int K, hipStream_t st);
// D6: PnPsolver::Refine on the inliers of masks row `row` (EPnP over them, CheckInliers of the
// refined pose: count in result[6], mask in row `row_out`, pose in Rt)
void launch_p4p_refine(PnPObject* d_obj, int row, int row_out, hipStream_t st);
// PnPsolver::SetRansacParameters + iterate(n_iterations) on the GPU (mmt_pnpsolver_iterate's
// semantics, include/mmt.h; throws ArgError on bad arguments)
void pnpsolver_iterate_gpu(hipStream_t s, const mmt_pnpsolver_problem* pr, const int32_t* randi,
                           int n_draw_iters, int n_iterations, mmt_pnpsolver_state* st,
                           float* Tcw_out, uint8_t* inliers_out, int* n_inliers, int* pose_found,
                           int* no_more);

}  // namespace mmt
