/* include/mmt.h -- C-ABI of libmmt, the MI355X-native per-frame front end of the
 * cule/multimot_track multi-motion tracker (ORB extraction -> flow/semantic association ->
 * per-motion pose solves).
 *
 * Plain pointers and sizes only; no OpenCV/Eigen/torch types.  Every entry point returns 0 on
 * success and a negative errno-style code on failure (never exit()); mmt_last_error() gives the
 * message.  One context per host thread, bound to one HIP device.  Inputs are caller-owned and
 * read-only (the reference mutates depthmap in place, Tracking.cc:447-456; we do not).
 *
 * Reference interfaces replaced (paths relative to the reference checkout):
 *   mmt_create          <- ORB_SLAM2::System::System(voc, settings, RGBD, viewer)  System.h:62,
 *                          Tracking::Tracking settings parse Tracking.cc:135-238,
 *                          ORBextractor::ORBextractor  ORBextractor.cc:410-470
 *   mmt_orb_extract     <- ORBextractor::operator()(image, mask, keypoints, descriptors)
 *                          ORBextractor.h:59-61 / ORBextractor.cc:1046-1109
 *   mmt_orb_extract_batch / _device
 *                       <- the same, over many frames (ORB extraction is stateless per frame)
 *   mmt_track_rgbd      <- System::TrackRGBD(im, depthmap, flowmap, masksem, ...) System.h:73-75,
 *                          System.cc:169-220 -> Tracking::GrabImageRGBD Tracking.cc:438-919
 *   mmt_track_rgbd_chunk / _chunk_device
 *                       <- the same over consecutive frames of the sequence (rgbd_tum.cc:158-176
 *                          calls it once per frame; frames of one sequence are a strict chain,
 *                          only ORB extraction is batched)
 *   mmt_pose_flow_solve <- Optimizer::PoseOptimizationFlow2Cam / PoseOptimizationFlow2
 *                          Optimizer.h:43-56, Optimizer.cc:396-601 / 2170-2377
 *   mmt_pose_optimization <- Optimizer::PoseOptimization(Frame*) Optimizer.cc:3121-3339
 *   mmt_frame_grid      <- Frame::ComputeStereoFromRGBD + AssignFeaturesToGrid Frame.cc:1041, 601
 *   mmt_search_by_projection_frame
 *                       <- ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono)
 *                          ORBmatcher.h / ORBmatcher.cc:1958-2102
 *   mmt_search_local_points
 *                       <- Tracking::SearchLocalPoints Tracking.cc:3416-3466 ->
 *                          ORBmatcher::SearchByProjection(Frame&, vector<MapPoint*>, th) :418-502
 *   mmt_search_by_bow   <- ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&, ...)
 *                          ORBmatcher.cc:532-663 (TrackReferenceKeyFrame Tracking.cc:2841-2853,
 *                          Relocalization :3631-3651)
 *   mmt_search_by_projection_keyframe
 *                       <- ORBmatcher::SearchByProjection(Frame&, KeyFrame*, const set<MapPoint*>&,
 *                          th, ORBdist) ORBmatcher.cc:2104-2231 (Relocalization :3717-3745)
 *   mmt_search_for_triangulation
 *                       <- LocalMapping::ComputeF12 + ORBmatcher::SearchForTriangulation
 *                          ORBmatcher.cc:1032-1131 (CreateNewMapPoints LocalMapping.cc:253-264)
 *   mmt_fuse_candidates <- ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th)'s search,
 *                          ORBmatcher.cc:1200-1324 (LocalMapping::SearchInNeighbors
 *                          LocalMapping.cc:458-538)
 *   mmt_local_bundle_adjustment
 *                       <- Optimizer::LocalBundleAdjustment's two optimisation rounds and inlier
 *                          test, Optimizer.cc:3394-3631 (LocalMapping.cc:81-84)
 *   mmt_load_vocabulary <- System::System's mpVocabulary->loadFromTextFile(strVocFile)
 *                          System.cc:63-73 (TemplatedVocabulary::loadFromTextFile,
 *                          Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1338-1424)
 *   mmt_bow_transform   <- TemplatedVocabulary::transform(feature, word, weight, &node, levelsup)
 *                          TemplatedVocabulary.h:1218-1259 (Frame::ComputeBoW, Frame.cc:778-786)
 *   mmt_train_vocabulary <- TemplatedVocabulary::create(training_features, k, L, weighting,
 *                          scoring) TemplatedVocabulary.h:558-616 (HKmeansStep :642-819,
 *                          initiateClustersKMpp :833-913, setNodeWeights :943-996)
 *   mmt_save_vocabulary <- TemplatedVocabulary::saveToTextFile TemplatedVocabulary.h:1429-1449
 *   mmt_stereo_frame    <- System::TrackStereo -> Tracking::GrabImageStereo's stereo Frame
 *                          constructor Frame.cc:79-159
 *   mmt_stereo_matches  <- Frame::ComputeStereoMatches Frame.cc:849-1038
 *   mmt_search_by_bow_keyframes
 *                       <- ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vector<MapPoint*>&)
 *                          ORBmatcher.cc:897-1030 (LoopClosing::ComputeSim3 LoopClosing.cc:254-282),
 *                          a batch of candidates
 *   mmt_sim3solver_iterate
 *                       <- Sim3Solver::SetRansacParameters + iterate, Sim3Solver.cc:114-364
 *                          (LoopClosing::ComputeSim3 LoopClosing.cc:276-303), a batch of solvers
 *   mmt_search_by_sim3  <- ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th)
 *                          ORBmatcher.cc:1477-1701 (LoopClosing.cc:325)
 *   mmt_optimize_sim3   <- Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale)
 *                          Optimizer.cc:3934-4129 (LoopClosing.cc:327), a batch of candidates
 *   mmt_detect_loop     <- LoopClosing::DetectLoop LoopClosing.cc:105-231
 *   mmt_detect_loop_candidates
 *                       <- KeyFrameDatabase::DetectLoopCandidates KeyFrameDatabase.cc:76-197
 *   mmt_loop_db_add / _erase
 *                       <- KeyFrameDatabase::add / erase KeyFrameDatabase.cc:40-68
 *   mmt_destroy         <- System::Shutdown / delete
 */
#ifndef MMT_H
#define MMT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMT_OK 0
#define MMT_EINVAL (-22)
#define MMT_ENOMEM (-12)
#define MMT_ENOSPC (-28)
#define MMT_EDEVICE (-5)
#define MMT_ESTATE (-77)

/* Most object motions a frame reports (semantic labels 1..15).  mmt_frame_result.n_objects is
 * the frame's full count; an objs_cap below it receives the first objs_cap motions only, so size
 * the motion arrays with MMT_MAX_OBJECTS per frame. */
#define MMT_MAX_OBJECTS 15

/* Settings of kitti03.yaml (Camera.*, ThDepth, ORBextractor.*) plus build-side knobs. */
typedef struct mmt_config {
  int width, height;              /* Camera.width / Camera.height                       */
  float fx, fy, cx, cy;           /* Camera.fx fy cx cy                                  */
  float k1, k2, p1, p2, k3;       /* distortion (must be 0 on this path)                 */
  float bf;                       /* Camera.bf                                           */
  float th_depth;                 /* ThDepth (baseline units, Tracking.cc:225)          */
  int rgb;                        /* Camera.RGB (1: cvtColor RGB2GRAY on the input)      */
  int orb_nfeatures;              /* ORBextractor.nFeatures                              */
  float orb_scale_factor;         /* ORBextractor.scaleFactor                            */
  int orb_nlevels;                /* ORBextractor.nLevels                                */
  int orb_ini_th_fast;            /* ORBextractor.iniThFAST                              */
  int orb_min_th_fast;            /* ORBextractor.minThFAST                              */
  uint32_t noise_seed;            /* replaces cv::RNG(time(NULL)), Frame.cc:1246         */
  int device_id;                  /* HIP device ordinal                                  */
  int max_batch;                  /* frames in flight for batched ORB extraction         */
  float fps;                      /* Camera.fps: mMaxFrames of the keyframe policy
                                     (Tracking.cc:170-176; 0 -> 30 as the reference)     */
} mmt_config;

/* cv::KeyPoint, same field order and size (28 bytes). */
typedef struct mmt_kp {
  float x, y, size, angle, response;
  int32_t octave, class_id;
} mmt_kp;

/* One recovered object motion (Tracking.cc:2127-2129: vObjMod = Tcw^-1 * X). */
typedef struct mmt_motion {
  int32_t label;            /* nModLabel (track id)                                   */
  int32_t sem_label;        /* semantic label (nSemPosition)                          */
  int32_t n_points;         /* object samples (ObjIdNew[i].size())                    */
  int32_t n_inliers;        /* solve edges with chi2 <= 0.01 after PoseOptimizationFlow2 */
  int32_t n_ransac_inliers; /* solvePnPRansac inliers                                 */
  int32_t n_mm_inliers;     /* motion-model inliers (-1: no previous motion)          */
  int32_t n_solve;          /* flow vertices in the solve (ObjIdTest_in.size())        */
  int32_t iterations;       /* LM iterations                                          */
  float world_motion[16];   /* row-major 4x4 vObjMod = Tcw^-1 * X                      */
  float cam_pose[16];       /* row-major 4x4 X (PoseOptimizationFlow2 output)          */
  float init_pose[16];      /* row-major 4x4 mInitModel (PnP or motion model)          */
  float centre_pre[3];      /* ObjCentre3D_pre (Tracking.cc:2032-2049): mean world point of
                               the solve's last-frame samples, noisy depth (UnprojectStereoObject
                               (j, 1)); the object-speed estimate of Tracking.cc:2186 uses it.
                               The reference computes it before the solve whatever the count:
                               1-2 samples give their mean, none gives NaN (0 * (1 / 0))   */
} mmt_motion;

/* Per-frame tracking result (the Tcw cv::Mat returned by System::TrackRGBD + counters). */
typedef struct mmt_frame_result {
  float Tcw[16];            /* row-major camera pose (world -> camera)                 */
  int32_t initialized;      /* tracking state OK (StereoInitialization done)           */
  int32_t n_keypoints;      /* ORB keypoints of the frame                              */
  int32_t n_obj_samples;    /* mvObjKeys.size(): last frame's hand-off (own on frame 0) */
  int32_t ego_iterations;   /* LM iterations of PoseOptimizationFlow2Cam               */
  int32_t ego_inliers;      /* its inliers (chi2 <= 0.04)                              */
  int32_t n_objects;        /* dynamic objects solved this frame                       */
  /* ORB-SLAM2 map tracking (Tracking.cc:985-1176), which sets the flow solve's initial pose */
  int32_t map_state;        /* mState after the frame: 0 not initialised, 1 OK, 2 LOST     */
  int32_t map_matches_mm;   /* TrackWithMotionModel's SearchByProjection matches (-1: none) */
  int32_t map_inliers_local;/* mnMatchesInliers of TrackLocalMap (-1: not run)             */
  int32_t n_keyframes;      /* keyframes in the map                                      */
  int32_t n_mappoints;      /* map points in the map                                     */
  int32_t new_keyframe;     /* this frame became a keyframe                              */
  float Tcw_map[16];        /* row-major pose of the map branch (PoseOptimization's output,
                               the initial estimate of PoseOptimizationFlow2Cam)        */
  int32_t frame_index;      /* this frame's index in the sequence (frames since the reset) */
  int32_t objects_frame;    /* the frame whose object motions n_objects / objs describe: this
                               frame, or with deferred object results an earlier one (-1:
                               none in this slot)                                        */
} mmt_frame_result;

typedef struct mmt_ctx mmt_ctx;

int mmt_version(void);
const char* mmt_last_error(const mmt_ctx* ctx);

mmt_ctx* mmt_create(const mmt_config* cfg);
void mmt_destroy(mmt_ctx* ctx);

/* Per-level ORB tables derived exactly as ORBextractor's ctor (sizes nlevels). */
int mmt_orb_levels(const mmt_ctx* ctx, float* scale, float* sigma2, int* n_per_level,
                   int* level_w, int* level_h);

/* ORBextractor::operator() on one 8-bit gray image (host pointers). keypoints/descriptors are
 * level-major exactly as the reference.  *n receives the count; MMT_ENOSPC if cap is short. */
int mmt_orb_extract(mmt_ctx* ctx, const uint8_t* gray, int w, int h, int stride, mmt_kp* kps,
                    uint8_t* desc, int cap, int* n);

/* Same over `nframes` host frames (each w x h, row stride `stride`), processed as one batch
 * of device launches.  Outputs are frame-major with `cap_per_frame` slots per frame. */
int mmt_orb_extract_batch(mmt_ctx* ctx, const uint8_t* const* grays, int nframes, int stride,
                          mmt_kp* kps, uint8_t* desc, int cap_per_frame, int* n_per_frame);

/* Device-resident variant: d_gray holds nframes gray frames (pitch frame_pitch bytes, rows of
 * `width` bytes, tightly packed); all outputs are device pointers; runs on `stream`
 * (hipStream_t, may be NULL for the context stream).  No host synchronisation, so the device-side
 * error flags of these launches are reported by mmt_orb_device_status. */
int mmt_orb_extract_device(mmt_ctx* ctx, const uint8_t* d_gray, int nframes, size_t frame_pitch,
                           mmt_kp* d_kps, uint8_t* d_desc, int cap_per_frame, int* d_n,
                           void* stream);

/* Synchronises `stream` (NULL: the context stream) and reports the device-side error flags that
 * ORB launches set since the last check (octree pass guard, node capacity, output truncation):
 * MMT_OK, or MMT_EDEVICE with mmt_last_error naming the flags.  The flags are cleared.  The
 * synchronous entry points (mmt_orb_extract*, mmt_track_rgbd*) run this check themselves, so a
 * tripped guard is never returned as MMT_OK with truncated keypoints. */
int mmt_orb_device_status(mmt_ctx* ctx, void* stream);

/* System::TrackRGBD on one frame (host buffers): bgr 8UC3 (w*h*3), disparity*256 u16 (w*h),
 * flow t->t+1 (w*h*2 float), semantic labels (w*h int32, LoadMask-filtered).  Fills `res` and up
 * to objs_cap object motions.  The first call with > 500 keypoints initialises (Tcw = I). */
int mmt_track_rgbd(mmt_ctx* ctx, const uint8_t* bgr, const uint16_t* disp256,
                   const float* flow_uv, const int32_t* mask, double timestamp,
                   mmt_frame_result* res, mmt_motion* objs, int objs_cap);

/* System::TrackRGBD over nframes consecutive frames in host memory, one pointer per frame and
 * input (layouts as mmt_track_rgbd): the frames are staged on the device and tracked as one chunk
 * (batched ORB, then frame by frame), like mmt_track_rgbd_chunk_device.  nframes <=
 * config.max_batch; res[nframes], objs[nframes * objs_cap].  Frames in pinned memory from
 * mmt_host_alloc reach the GPU by DMA at full PCIe rate. */
int mmt_track_rgbd_chunk(mmt_ctx* ctx, int nframes, const uint8_t* const* bgr,
                         const uint16_t* const* disp256, const float* const* flow_uv,
                         const int32_t* const* mask, mmt_frame_result* res, mmt_motion* objs,
                         int objs_cap);

/* Page-locked host memory on the context's device (hipHostMalloc), for frames the caller decodes
 * and hands to the host-buffer entry points.  NULL on failure; release with mmt_host_free. */
void* mmt_host_alloc(mmt_ctx* ctx, size_t bytes);
void mmt_host_free(mmt_ctx* ctx, void* p);

/* Device-resident chunk of consecutive frames of the context's sequence (pitches in bytes):
 * ORB extraction is batched over the chunk, tracking then runs frame by frame.  res[nframes],
 * objs[nframes * objs_cap] are host arrays.
 * Errors (both track entry points): a chunk whose ORB run trips a device guard returns
 * MMT_EDEVICE before any of its frames is tracked, and the context keeps the state of the previous
 * call, so tracking may continue with the next frames (or restart after mmt_reset). */
int mmt_track_rgbd_chunk_device(mmt_ctx* ctx, int nframes, const uint8_t* d_bgr,
                                size_t bgr_pitch, const uint16_t* d_disp, size_t disp_pitch,
                                const float* d_flow, size_t flow_pitch, const int32_t* d_mask,
                                size_t mask_pitch, mmt_frame_result* res, mmt_motion* objs,
                                int objs_cap, void* stream);

/* One flow-refined pose solve (probe of PoseOptimizationFlow2Cam / PoseOptimizationFlow2).
 * obs/flow: n x 2 floats (last-frame sample pixel, its flow); depth: n floats. */
typedef struct mmt_flow_problem {
  int n;
  const float* obs;
  const float* flow;
  const float* depth;
  float Tcw_last[16];  /* row-major last camera pose; edges use its inverse (Twl)   */
  float init[16];      /* row-major initial estimate                                */
  float rp_thres;      /* 0.04 ego / 0.01 object (Huber delta^2)                    */
  double prior_info;   /* 0.3 ego / 0.5 object                                      */
  int max_iters;       /* 100 ego / 200 object                                      */
  int use_noise;       /* ego: depth += g0 * z^2/362.5*0.15 (ObtainFlowDepthCamera) */
  float g0;            /* the cv::RNG gaussian draw of the noise seed               */
  float fx, fy, cx, cy;
} mmt_flow_problem;
int mmt_pose_flow_solve(mmt_ctx* ctx, const mmt_flow_problem* problem, float* pose_out,
                        int* stats_out /* iterations, inliers, status */);
/* The same solve with the initial pose read from device memory (init_on_device != 0: the path of
 * the tracker's ego solve queued behind PoseOptimization) and, optionally, the mean world
 * position of the solve's points (centre_out: 3 floats or null). */
int mmt_pose_flow_solve_init_dev(mmt_ctx* ctx, const mmt_flow_problem* problem,
                                 int init_on_device, float* pose_out, int* stats_out,
                                 float* centre_out);

/* Optimizer::PoseOptimization(Frame*) (reference include/Optimizer.h:43, src/Optimizer.cc:3121-3339)
 * on the frame's MapPoint observations (the edges of the frame's non-null mvpMapPoints, in index
 * order): Xw n x 3 world positions, obs n x (u, v, uR) with uR = mvuRight (< 0: mono edge),
 * inv_sigma2 n = mvInvLevelSigma2[octave].  Tcw = pFrame->mTcw (row-major).  Writes the optimised
 * pose and mvbOutlier (outlier_out, n bytes); *n_inliers = the function's return value
 * (nInitialCorrespondences - nBad; 0 with the pose unchanged below 3 edges). */
typedef struct mmt_pose_opt_problem {
  int n;
  const float* Xw;
  const float* obs;
  const float* inv_sigma2;
  float Tcw[16];
  float fx, fy, cx, cy, bf;
} mmt_pose_opt_problem;
int mmt_pose_optimization(mmt_ctx* ctx, const mmt_pose_opt_problem* problem, float* pose_out,
                          uint8_t* outlier_out, int* n_inliers);

/* cv::solvePnPRansac(..., SOLVEPNP_AP3P) probe as called by GetInitModelObj: pts3 n x 3,
 * pts2 n x 2 floats.  R_out row-major 3x3 (after the Rodrigues round trip), t_out 3;
 * inliers_out (optional, n ints) receives the RANSAC inlier indices. */
int mmt_pnp_ransac(mmt_ctx* ctx, const float* pts3, const float* pts2, int n, float fx,
                   float fy, float cx, float cy, int max_iters, double reproj, double confidence,
                   double* R_out, double* t_out, int* inliers_out, int* n_inliers,
                   int* iters_out /* iterations run, best hypothesis */);

/* ---- PnPsolver (row D6): ORB-SLAM2's P4P EPnP-RANSAC of Tracking::Relocalization -------------
 * PnPsolver(F, vpMapPointMatches) + SetRansacParameters(probability, minInliers, maxIterations,
 * minSet, epsilon, th2) + iterate(nIterations, bNoMore, vbInliers, nInliers) (reference
 * src/PnPsolver.cc:67-339, driven by Tracking.cc:3659-3700 with (0.99, 10, 300, 4, 0.5, 5.991)
 * and nIterations 5).  The n correspondences in mvP2D / mvP3Dw order: pts3 n x 3 world points,
 * pts2 n x 2 pixels (mvKeysUn), sigma2 n = mvLevelSigma2[octave].  min_set must be 4.
 *
 * Random minimal sets: the reference draws them with DUtils::Random::RandomInt (rand()), so the
 * caller keeps that stream.  randi[4 k + j] = RandomInt(0, n - 1 - j) of draw j in iteration k of
 * this call; n_draw_iters must cover the call: max(maxIts - state->iterations, n_iterations),
 * maxIts being the iteration cap SetRansacParameters derives.  The solver's state across calls
 * (mnIterations, mnBestInliers, mBestTcw, mvbBestInliers) is *state, caller-owned (best_mask: n
 * bytes); zero it (iterations = best_inliers = 0) for a new solver.
 *
 * Outputs: *pose_found = 1 and Tcw_out / inliers_out (n bytes, mvKeyPointIndices order) /
 * *n_inliers when iterate() returns a pose (refined, or the best hypothesis once the iterations
 * are exhausted), 0 for the reference's empty cv::Mat; *no_more = bNoMore. */
typedef struct mmt_pnpsolver_problem {
  int n;
  const float* pts3;
  const float* pts2;
  const float* sigma2;
  float fx, fy, cx, cy;
  double probability;
  int min_inliers;
  int max_iterations;
  int min_set;
  float epsilon;
  float th2;
} mmt_pnpsolver_problem;

typedef struct mmt_pnpsolver_state {
  int iterations;          /* mnIterations                                                 */
  int best_inliers;        /* mnBestInliers                                                */
  float best_Tcw[16];      /* mBestTcw (row-major)                                         */
  uint8_t* best_mask;      /* mvbBestInliers, n bytes                                      */
} mmt_pnpsolver_state;

int mmt_pnpsolver_iterate(mmt_ctx* ctx, const mmt_pnpsolver_problem* problem,
                          const int32_t* randi, int n_draw_iters, int n_iterations,
                          mmt_pnpsolver_state* state, float* Tcw_out, uint8_t* inliers_out,
                          int* n_inliers, int* pose_found, int* no_more);

/* ---- Frame grid and projection matching (rows B3, C1-C3 of the hot path) ----------------------
 * The current Frame as the matchers read it: its ORB keys (mvKeysUn == mvKeys, no distortion),
 * descriptors (n x 32) and the metric depth map (w x h floats, the Tcw-independent part of
 * Frame::ComputeStereoFromRGBD).  Camera intrinsics, bf and the scale pyramid come from the
 * context's configuration; image bounds are [0, width] x [0, height] (Frame::ComputeImageBounds). */
typedef struct mmt_match_frame {
  int n;
  const mmt_kp* kps;
  const uint8_t* desc;
  const float* depth;
  float Tcw[16];        /* row-major mTcw used for the projections                         */
} mmt_match_frame;

/* Frame::ComputeStereoFromRGBD + AssignFeaturesToGrid (Frame.cc:1041-1062, 601-616, PosInGrid
 * 765-775): uR_out/depth_out (n) = mvuRight/mvDepth (-1 without depth); the 64 x 48 grid mGrid as
 * CSR: cell (ix, iy) holds cell_idx[cell_start[ix*48+iy] .. cell_start[ix*48+iy+1]) in ascending
 * key order; cell_start has 3073 entries, cell_idx n.  n <= 16384. */
int mmt_frame_grid(mmt_ctx* ctx, const mmt_match_frame* cur, float* uR_out, float* depth_out,
                   int* cell_start, int* cell_idx);

/* The last Frame as ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono) reads it:
 * per last-frame key i, its keypoint (octave, angle), the world position and descriptor of
 * mvpMapPoints[i], and active[i] = (mvpMapPoints[i] != NULL && !mvbOutlier[i]). */
typedef struct mmt_last_frame {
  int n;
  const mmt_kp* kps;
  const float* Xw;          /* n x 3 */
  const uint8_t* mp_desc;   /* n x 32 */
  const uint8_t* active;    /* n */
  float Tcw[16];            /* row-major LastFrame.mTcw */
  const uint8_t* obs;       /* n, optional: mvpMapPoints[i]->Observations() > 0.  A current key
                               bound to a point without observations (a temporal visual-odometry
                               point of UpdateLastFrame) stays open to later points (NULL: every
                               point has observations) */
} mmt_last_frame;

/* ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono) with mbCheckOrientation
 * (ORBmatcher.cc:1958-2102, called by Tracking::TrackWithMotionModel Tracking.cc:2962-3010; C1
 * DescriptorDistance ORBmatcher.cc:2279-2295).  The current frame starts with no MapPoints (as
 * after the fill(NULL) of Tracking.cc:2975); match_out[i2] (cur->n) = the last-frame index bound
 * to current key i2, or -1; *nmatches = the function's return value. */
int mmt_search_by_projection_frame(mmt_ctx* ctx, const mmt_match_frame* cur,
                                   const mmt_last_frame* last, float th, int mono,
                                   int check_orientation, int32_t* match_out, int* nmatches);

/* Local MapPoints as Tracking::SearchLocalPoints sees them (Tracking.cc:3416-3466): position,
 * mNormalVector, mfMinDistance / mfMaxDistance, mDescriptor, and skip = already matched in this
 * frame (mnLastFrameSeen == mCurrentFrame.mnId) or isBad(). */
typedef struct mmt_local_points {
  int m;
  const float* Xw;        /* m x 3  */
  const float* normal;    /* m x 3  */
  const float* min_dist;  /* m      */
  const float* max_dist;  /* m      */
  const uint8_t* desc;    /* m x 32 */
  const uint8_t* skip;    /* m      */
} mmt_local_points;

/* SearchLocalPoints' projection pass (Frame::isInFrustum(pMP, 0.5), Frame.cc:652-708, with
 * MapPoint::PredictScale MapPoint.cc:402-417) + ORBmatcher(0.8)::SearchByProjection(Frame&,
 * vector<MapPoint*>, th) (ORBmatcher.cc:418-502).  taken (cur->n bytes, optional) marks keys
 * that already hold a MapPoint; match_out[i] (cur->n) = the local point newly bound to key i, or
 * -1; frustum_out (m x 6 floats, optional) = in_view, predicted level, u, v, uR, view cos. */
int mmt_search_local_points(mmt_ctx* ctx, const mmt_match_frame* cur,
                            const mmt_local_points* pts, float th, const uint8_t* taken,
                            int32_t* match_out, float* frustum_out, int* nmatches);

/* DBoW2::FeatureVector (std::map<NodeId, std::vector<unsigned int>>, FeatureVector.h) as flat
 * arrays: node_id ascending; the features of node k are feat[node_start[k] .. node_start[k+1])
 * in insertion order.  Every frame feature is listed in at most one node (DBoW2's transform puts
 * each feature in one node at the direct-index level), and a node holds at most 16384 of them
 * (a vocabulary of depth <= 4 files every feature of a frame under node 0). */
typedef struct mmt_feature_vector {
  int n_nodes;
  const uint32_t* node_id;    /* n_nodes              */
  const int32_t* node_start;  /* n_nodes + 1, from 0  */
  const int32_t* feat;        /* node_start[n_nodes]  */
} mmt_feature_vector;

/* A keyframe as SearchByBoW reads it: mvKeysUn (angle), mDescriptors, whether mvpMapPoints[i] holds
 * a MapPoint that is not bad, and mFeatVec. */
typedef struct mmt_bow_keyframe {
  int n;
  const mmt_kp* kps;
  const uint8_t* desc;      /* n x 32 */
  const uint8_t* mp_valid;  /* n      */
  mmt_feature_vector fv;
} mmt_bow_keyframe;

/* C4: ORBmatcher(nn_ratio, check_orientation)::SearchByBoW(pKF, F, vpMapPointMatches, ...)
 * (ORBmatcher.cc:532-663): per common vocabulary node, each keyframe feature with a good MapPoint
 * takes the closest unmatched frame feature of the node if its distance is <= TH_LOW (50) and below
 * nn_ratio times the second-best distance; then the rotation-consistency histogram.  match_out[i]
 * (n_cur) = the keyframe key whose MapPoint now matches frame key i (vpMapPointMatches[i] =
 * pKF->mvpMapPoints[match_out[i]]), or -1; *nmatches = the return value.  The reference uses
 * nn_ratio 0.7 in TrackReferenceKeyFrame and 0.75 in Relocalization. */
int mmt_search_by_bow(mmt_ctx* ctx, const mmt_bow_keyframe* kf, int n_cur, const mmt_kp* cur_kps,
                      const uint8_t* cur_desc, const mmt_feature_vector* cur_fv, float nn_ratio,
                      int check_orientation, int32_t* match_out, int* nmatches);

/* ORBmatcher(nn_ratio, check_orientation)::SearchByBoW(pKF1, pKF2, vpMatches12) ORBmatcher.cc:897-1030
 * for one keyframe 1 against n_cand keyframes 2 (LoopClosing.cc:254-282), one call.
 * match12_out[c * kf1->n + i1] = the key of candidate c whose MapPoint matches key i1 of keyframe 1
 * (vpMatches12[i1] = pKF2->mvpMapPoints[that key]) or -1; nmatches_out[c] = the return value.
 * Unlike C4: the distance must be < TH_LOW (strict), a key of keyframe 2 without a good MapPoint is
 * never scanned, and the rotation is keyframe 1's angle minus keyframe 2's.  n_cand <= 64; a
 * feature may be listed once only in either keyframe's vector, and a node of a candidate holds at
 * most 16384 features (MMT_EINVAL otherwise).  LoopClosing uses nn_ratio 0.75 with the orientation
 * check and discards a candidate at nmatches < 20. */
int mmt_search_by_bow_keyframes(mmt_ctx* ctx, const mmt_bow_keyframe* kf1, int n_cand,
                                const mmt_bow_keyframe* kf2 /* n_cand */, float nn_ratio,
                                int check_orientation, int32_t* match12_out, int32_t* nmatches_out);

/* ORBmatcher::Fuse(pKF, vpMapPoints, th)'s per-point search (ORBmatcher.cc:1200-1324): the point
 * projected with the keyframe's pose (cur->Tcw), KeyFrame::IsInImage, the scale-invariance
 * distances (0.8 mfMinDistance, 1.2 mfMaxDistance), the 60-degree viewing angle, PredictScale, then
 * the keyframe keys in radius th * scale[level] at the predicted level or one below, gated by the
 * reprojection error (7.8 stereo, 5.99 monocular, times 1/sigma^2), and the closest descriptor
 * (first of equal distances).  best_idx / best_dist (m) = that key and its distance, or -1 / 256;
 * the reference fuses when best_dist <= 50.  The keyframe is a mmt_match_frame (its depth map
 * gives mvuRight); pts->skip is ignored (the caller skips bad points and points already in the
 * keyframe, ORBmatcher.cc:1224). */
int mmt_fuse_candidates(mmt_ctx* ctx, const mmt_match_frame* kf, const mmt_local_points* pts,
                        float th, int32_t* best_idx, int32_t* best_dist);

/* The graph of Optimizer::LocalBundleAdjustment (Optimizer.cc:3408-3541): keyframe vertices
 * (Tcw, fixed: the fixed cameras and keyframe 0), map points, and one edge per observation, listed
 * point by point (e_pt non-decreasing) with each point's observations in keyframe order. */
typedef struct mmt_ba_problem {
  int n_kf, n_pt, n_edge;
  const float* Tcw;            /* n_kf x 16 row-major                                  */
  const uint8_t* fixed;        /* n_kf                                                 */
  const float* Xw;             /* n_pt x 3                                             */
  const int32_t* e_pt;         /* n_edge                                               */
  const int32_t* e_kf;         /* n_edge                                               */
  const float* e_obs;          /* n_edge x (u, v, uR): keypoint and mvuRight (< 0: monocular,
                                  EdgeSE3ProjectXYZ; else EdgeStereoSE3ProjectXYZ)     */
  const float* e_inv_sigma2;   /* n_edge: mvInvLevelSigma2[octave] (the information)   */
} mmt_ba_problem;

/* LocalBundleAdjustment's solve (Optimizer.cc:3547-3631; g2o LM with BlockSolver_6_3, Huber
 * sqrt(5.991) / sqrt(7.815) in the first 5 iterations, the bad edges set aside, 10 more without the
 * kernel) on the GPU.  Tcw_out (n_kf x 16) and Xw_out (n_pt x 3) = Converter::toCvMat of the final
 * estimates; erase_out (n_edge) = the final inlier test failed (the observation the reference
 * erases); stats (5) = iterations of round 1, of round 2, LM trials of round 1, of round 2, erased
 * edges.  Camera from the context's configuration. */
int mmt_local_bundle_adjustment(mmt_ctx* ctx, const mmt_ba_problem* problem, float* Tcw_out,
                                float* Xw_out, uint8_t* erase_out, int32_t* stats);

/* LocalMapping counters of the context's tracker (no reference counterpart: test and profiling
 * hook).  Times are host wall microseconds, collected with MMT_MAP_PROFILE=1. */
typedef struct mmt_map_counters {
  int64_t n_ba, n_fused, n_culled, n_ba_erased, ba_trials, ba_edges, ba_kfs, ba_pts, ba_max_opt,
      fuse_launches, fuse_queries, fuse_relaunches;
  double lm_us, ba_us, fuse_us;
  int64_t d2_split_fallbacks;  /* ego flow solves re-run on one workgroup because the split
                                  solve's workgroups were not resident together             */
  int64_t n_reparent;          /* spanning-tree children re-parented by KeyFrame::SetBadFlag
                                  (KeyFrame.cc:480-537) when KeyFrameCulling culls a keyframe */
} mmt_map_counters;
int mmt_map_counters_read(mmt_ctx* ctx, mmt_map_counters* out);

/* Test knob (no reference counterpart): LocalMapping::KeyFrameCulling's redundancy ratio, a
 * keyframe is culled when more than ratio x its close map points are seen by 3 other keyframes
 * (0.9 in the reference, LocalMapping.cc:697; the default).  The synthetic sequences never reach
 * 0.9, so the culling tests lower it to exercise KeyFrame::SetBadFlag. */
int mmt_set_keyframe_culling_ratio(mmt_ctx* ctx, double ratio);

/* ---- ORB vocabulary ------------------------------------------------------------
 * System(voc, ...) loads DBoW2's text vocabulary (System.cc:63-73): the header "k L scoring
 * weighting", then one line per node "parent is_leaf d0 .. d31 weight".  With a vocabulary the
 * tracker runs the reference's TrackReferenceKeyFrame (SearchByBoW against the reference
 * keyframe, Tracking.cc:2836-2892), Relocalization (KeyFrameDatabase candidates, SearchByBoW,
 * PnPsolver, the SearchByProjection(F, KF, ...) rounds; Tracking.cc:3614-3776) and LocalMapping's
 * CreateNewMapPoints (SearchForTriangulation, LocalMapping.cc:210-456), and keeps the keyframe
 * database; without one it runs the documented substitutes.  Load it before
 * the first frame (MMT_ESTATE afterwards).  Scorings L1 / L2 (ORBvoc.txt: L1, TF-IDF); errors:
 * MMT_EINVAL with mmt_last_error (unreadable file, the reference's header check). */
int mmt_load_vocabulary(mmt_ctx* ctx, const char* path);

/* Probe of TemplatedVocabulary::transform(feature, id, w, &nid, levelsup) over n descriptors (host
 * n x 32) on the GPU: word id, word weight (0: stopped) and the node at level L - levelsup. */
int mmt_bow_transform(mmt_ctx* ctx, const uint8_t* desc, int n, int levelsup, uint32_t* word,
                      double* weight, uint32_t* node);

/* ---- training a vocabulary ------------------------------------------------------------------------
 * TemplatedVocabulary::create(training_features, k, L, weighting, scoring) on the GPU: hierarchical
 * k-medians (k-means++ seeding, Lloyd iterations with FORB::meanValue's bit majority) level by
 * level, then setNodeWeights.  Every decision is an integer, so the tree is bit-identical to a
 * sequential run of the reference's steps.  Pinned where the reference leaves a choice (DESIGN.md
 * section 2): the random stream (seed; the reference seeds rand() from the wall clock), an emptied
 * cluster keeps its centre, max_iters caps the Lloyd iterations of a level. */
typedef struct mmt_voc_train_params {
  int k, L;            /* branching factor 2..20, depth 1..10 (the loader's limits; k >= 2)     */
  int weighting;       /* DBoW2 WeightingType: 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY                  */
  int scoring;         /* DBoW2 ScoringType: 0 L1_NORM, 1 L2_NORM (what the loader accepts)     */
  uint64_t seed;       /* replaces SeedRandOnce()'s wall clock                                  */
  int max_iters;       /* cap on Lloyd iterations per level, 0 -> 1000                          */
} mmt_voc_train_params;
typedef struct mmt_voc_train_stats {
  int32_t n_nodes;          /* nodes of the tree, the root included                             */
  int32_t n_words;          /* leaves                                                           */
  int32_t n_kmeans_nodes;   /* nodes with more than k features (k-means ran)                    */
  int32_t n_capped;         /* nodes whose assignment still changed at max_iters                */
  int32_t n_empty_clusters; /* clusters left without a feature (childless nodes)                */
  int32_t iters[10];        /* Lloyd iterations run at tree level 1..L                          */
} mmt_voc_train_stats;
/* desc is image_start[n_images] x 32 bytes on the host, image i owning rows [image_start[i],
 * image_start[i + 1]).  Installs the result as the context's vocabulary, with full-precision
 * weights, under mmt_load_vocabulary's rule (MMT_ESTATE once the map has a keyframe).  MMT_EINVAL:
 * no descriptors or images, k or L out of range, a scoring above 1, a decreasing image_start. */
int mmt_train_vocabulary(mmt_ctx* ctx, const uint8_t* desc, const int32_t* image_start,
                         int n_images, const mmt_voc_train_params* params,
                         mmt_voc_train_stats* stats);

/* TemplatedVocabulary::saveToTextFile of the context's vocabulary (trained or loaded): the header
 * "k L  scoring weighting", one line per node in id order "parent leaf d0 .. d31  weight" with the
 * weight in six significant digits.  MMT_EINVAL without a vocabulary or when the file cannot be
 * written. */
int mmt_save_vocabulary(mmt_ctx* ctx, const char* path);

/* The keyframe's map points as Relocalization's SearchByProjection reads them, in the keyframe's
 * mvpMapPoints order: world position, mfMinDistance / mfMaxDistance, mDescriptor and the angle of
 * the keyframe key that holds the point (pKF->mvKeysUn[i].angle). */
typedef struct mmt_keyframe_points {
  int m;
  const float* Xw;        /* m x 3  */
  const float* min_dist;  /* m      */
  const float* max_dist;  /* m      */
  const uint8_t* desc;    /* m x 32 */
  const float* angle;     /* m      */
} mmt_keyframe_points;

/* Probe of ORBmatcher(0.9, true)::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist)
 * (ORBmatcher.cc:2104-2231) as Relocalization runs it: the code of the tracking path on
 * caller-supplied arrays.  cur: the current frame and its pose; skip (m bytes) marks points that
 * are bad or in sAlreadyFound; bound_in (cur->n bytes) marks current keys that hold a MapPoint when
 * the call starts.  match_out[i] (cur->n) = the point (index into points) newly bound to key i, or
 * -1, after the rotation histogram; *nmatches = the return value; *n_rescan (optional) = points
 * whose 32 listed candidates were all bound by earlier points, so that the host rescanned their
 * window. */
int mmt_search_by_projection_keyframe(mmt_ctx* ctx, const mmt_match_frame* cur,
                                      const mmt_keyframe_points* points, const uint8_t* skip,
                                      float th, int orb_dist, const uint8_t* bound_in,
                                      int32_t* match_out, int* nmatches, int* n_rescan);

/* ---- Loop-closure geometry: LoopClosing::ComputeSim3's steps 2 and 3 (LoopClosing.cc:227-420) ---
 * Sim3Solver(pKF1, pKF2, vpMatched12, bFixScale) + SetRansacParameters(probability, minInliers,
 * maxIterations) + iterate(nIterations, bNoMore, vbInliers, nInliers) (reference
 * src/Sim3Solver.cc:37-364; ComputeSim3 uses (0.99, 20, 300) and rounds of iterate(5) over its
 * candidate keyframes), for a batch of independent solvers: one call runs one round of every
 * candidate.  At most 64 solvers, 16384 correspondences per solver and 300 iterations per call.
 *
 * A problem holds the constructor's products in correspondence order (the order of mvX3Dc1):
 * X1 / X2 n x 3 = mvX3Dc1 / mvX3Dc2 (the matched points in camera 1 / camera 2), sigma2_1 /
 * sigma2_2 n = mvLevelSigma2[octave] of the two keys, the two cameras and bFixScale.  The entry
 * point derives mvnMaxError1 / 2 (9.210 sigma2 as the reference's vector<size_t> holds it) and
 * mvP1im1 / mvP2im2 (FromCameraToImage).
 *
 * Random minimal sets: randi[i][3 k + j] = DUtils::Random::RandomInt(0, n - 1 - j) of draw j in
 * iteration k of this call for solver i, the caller's stream as in mmt_pnpsolver_iterate;
 * n_draw_iters[i] must cover min(n_iterations, maxIts - state.iterations), maxIts being
 * SetRansacParameters' cap.  A solver with n < min_inliers returns no_more and reads no draw.
 *
 * The solver's state across calls (mnIterations, mnBestInliers, mBestT12, mBestRotation,
 * mBestTranslation, mBestScale, mvbBestInliers) is states[i], caller-owned (best_mask: n bytes);
 * zeroed it is a new solver.
 *
 * results[i]: found = iterate() returned a matrix, then T12 (row-major mBestT12), inliers (n
 * bytes, correspondence order; mapping through mvnIndices1 is the caller's) and n_inliers;
 * no_more = bNoMore.  probes (optional, n_solvers entries; test hook without a reference
 * counterpart): counts / flags (cap x n bytes) / T12 (cap x 16) of the first n_hyp <= cap
 * hypotheses the call launched for the solver, whether or not iterate()'s loop reached them.
 * Choices where the reference leaves the arithmetic to OpenCV: DESIGN.md section 2. */
typedef struct mmt_sim3_problem {
  int n;
  const float* X1;         /* n x 3 */
  const float* X2;         /* n x 3 */
  const float* sigma2_1;   /* n     */
  const float* sigma2_2;   /* n     */
  float fx1, fy1, cx1, cy1;  /* mK1 */
  float fx2, fy2, cx2, cy2;  /* mK2 */
  int fix_scale;           /* mbFixScale                                                   */
  double probability;      /* mRansacProb                                                  */
  int min_inliers;         /* mRansacMinInliers                                            */
  int max_iterations;      /* SetRansacParameters' maxIterations                           */
} mmt_sim3_problem;

typedef struct mmt_sim3_state {
  int iterations;          /* mnIterations                                                 */
  int best_inliers;        /* mnBestInliers                                                */
  float best_T12[16];      /* mBestT12 (row-major)                                         */
  float best_R[9];         /* mBestRotation                                                */
  float best_t[3];         /* mBestTranslation                                             */
  float best_scale;        /* mBestScale                                                   */
  uint8_t* best_mask;      /* mvbBestInliers, n bytes                                      */
} mmt_sim3_state;

typedef struct mmt_sim3_result {
  int found, n_inliers, no_more;
  float T12[16];
  uint8_t* inliers;        /* n bytes */
} mmt_sim3_result;

typedef struct mmt_sim3_probe {
  int cap, n_hyp;
  int32_t* counts;         /* cap      */
  uint8_t* flags;          /* cap x n  */
  float* T12;              /* cap x 16 */
} mmt_sim3_probe;

int mmt_sim3solver_iterate(mmt_ctx* ctx, int n_solvers, const mmt_sim3_problem* problems,
                           const int32_t* const* randi, const int32_t* n_draw_iters,
                           int n_iterations, mmt_sim3_state* states, mmt_sim3_result* results,
                           mmt_sim3_probe* probes);

/* ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (ORBmatcher.cc:1477-1701;
 * LoopClosing.cc:325 with th 7.5).  Each keyframe is a mmt_match_frame (keys, descriptors, grid,
 * Tcw) with its map points in mvpMapPoints order (points->m == kf->n; angle unused) and a skip
 * byte per slot (empty, or the point is bad).  matched12_in (n1): -1 no prior match, k >= 0 a
 * match to the point at key k of keyframe 2, -2 a match to a point keyframe 2 does not hold (sets
 * vbAlreadyMatched1 only, :1514).  Every unmatched point of keyframe 1 is moved into camera 2
 * (R1w Xw + t1w, then sR21, t21) and searched among keyframe 2's keys, and the reverse: depth not
 * negative, KeyFrame::IsInImage, the scale-invariance distances on cv::norm of the camera-frame
 * point, PredictScale, the window th * scale[level], keys at the predicted level or one below, the
 * closest descriptor (first of equal distances) if its distance is <= TH_HIGH (100).  No
 * viewing-angle or reprojection-error test.  match_out[i1] (n1) = the keyframe-2 key whose point
 * is newly matched (both directions agree), else -1; *n_found = the return value; cand1_out (n1) /
 * cand2_out (n2), optional = vnMatch1 / vnMatch2 before the agreement pass.  Camera (pKF1's, as
 * the reference uses for both directions) and image bounds from the context's configuration. */
int mmt_search_by_sim3(mmt_ctx* ctx, const mmt_match_frame* kf1,
                       const mmt_keyframe_points* points1, const uint8_t* skip1,
                       const mmt_match_frame* kf2, const mmt_keyframe_points* points2,
                       const uint8_t* skip2, float s12, const float* R12, const float* t12,
                       float th, const int32_t* matched12_in, int32_t* match_out, int* n_found,
                       int32_t* cand1_out, int32_t* cand2_out);

/* Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale) (Optimizer.cc:3934-4129;
 * LoopClosing.cc:327 with th2 10), for a batch of independent candidates: one call serves every
 * candidate of a ComputeSim3 round whose Sim3Solver returned a similarity.  At most 64 problems and
 * 16384 correspondences per problem; the whole batch is one launch.
 *
 * A problem holds what the reference gathers per correspondence that passes :4000-4002, in
 * vpMatches1 order (vnIndexEdge, the map back to vpMatches1, is the caller's): X1c / X2c = the two
 * map points in their own cameras (R1w P3D1w + t1w, the float cv::Mat product), obs1 / obs2 = the
 * undistorted keys, inv_sigma2_1 / 2 = mvInvLevelSigma2[octave], the two cameras, bFixScale, th2
 * and gScm's constructor arguments (s12, R12 row-major, t12).  Everything is promoted to double.
 *
 * What runs is g2o's optimisation of the one free VertexSim3Expmap over two fixed-point edges per
 * correspondence (e12 = obs1 - cam_map1(project(S12 X2c)), e21 = obs2 - cam_map2(project(S12^-1
 * X1c)), information inv_sigma2 I, Huber delta sqrtf(th2) in both rounds): g2o's numeric Jacobian
 * (central difference at 1e-9), Sim3's exponential update from the left, a dense 7 x 7 LDLT and
 * OptimizationAlgorithmLevenberg inside ORB-SLAM2's SparseOptimizer::optimize.  optimize(5); every
 * pair with e12.chi2() > th2 || e21.chi2() > th2 is removed (n_bad); with fewer than 10 pairs left
 * the call returns 0 and leaves g2oS12 alone (second_round 0); otherwise optimize(n_bad > 0 ? 10 :
 * 5) on the pairs left, the same test again, and g2oS12 receives the estimate.  chi2() reads the
 * error of the last computeActiveErrors, which is the last trial's state.  No depth test: a point
 * mapped to z = 0 gives a non-finite error, which counts as an inlier and makes the trial rejected.
 *
 * results[i]: n_inliers = the return value; n_bad; second_round; (s, R, t) = g2oS12 after the call
 * (scale(), rotation().toRotationMatrix() row-major, translation()), the input promoted when
 * second_round is 0; kept (n bytes) = vpMatches1 still non-null (pairs cleared by the first test
 * stay cleared); chi2 (optional, n x 2) = e12 / e21 chi2() of every pair at the state of the last
 * test that ran (the pairs removed after round 1 are evaluated there too, beyond the reference, so
 * that kept can be checked against it); stats = iterations of round 1 / 2, LM trials of round 1 / 2
 * (diagnostic).  n == 0: nothing runs.  Pins: DESIGN.md section 2. */
typedef struct mmt_sim3_opt_problem {
  int n;
  const float* X1c;        /* n x 3 */
  const float* X2c;        /* n x 3 */
  const float* obs1;       /* n x 2: pKF1->mvKeysUn[i].pt  */
  const float* obs2;       /* n x 2: pKF2->mvKeysUn[i2].pt */
  const float* inv_sigma2_1;  /* n */
  const float* inv_sigma2_2;  /* n */
  float fx1, fy1, cx1, cy1;   /* pKF1->mK */
  float fx2, fy2, cx2, cy2;   /* pKF2->mK */
  int fix_scale;           /* bFixScale */
  float th2;
  float s12, R12[9], t12[3];  /* gScm's constructor arguments (LoopClosing.cc:327) */
} mmt_sim3_opt_problem;

typedef struct mmt_sim3_opt_result {
  int n_inliers;
  int n_bad;
  int second_round;
  double s, R[9], t[3];
  uint8_t* kept;           /* n bytes */
  double* chi2;            /* optional, n x 2 */
  int stats[4];
} mmt_sim3_opt_result;

int mmt_optimize_sim3(mmt_ctx* ctx, int n_problems, const mmt_sim3_opt_problem* problems,
                      mmt_sim3_opt_result* results);

/* A keyframe as SearchForTriangulation reads it: mvKeysUn, mDescriptors, mvuRight (< 0: monocular),
 * mFeatVec, whether mvpMapPoints[i] holds a MapPoint, and Tcw (row-major). */
typedef struct mmt_sft_keyframe {
  int n;
  const mmt_kp* kps;
  const uint8_t* desc;     /* n x 32 */
  const float* uR;         /* n      */
  const uint8_t* has_mp;   /* n      */
  mmt_feature_vector fv;
  float Tcw[16];
} mmt_sft_keyframe;

/* Probe of LocalMapping::CreateNewMapPoints' matching step (LocalMapping.cc:253-264): for each of
 * the n_pairs neighbours kf2[p], ComputeF12(kf1, kf2[p]) and ORBmatcher(0.6, false)::
 * SearchForTriangulation (ORBmatcher.cc:1032-1131), all pairs in one launch as on the tracking
 * path.  match12_out[p * kf1->n + i] = the key of kf2[p] matched to key i of kf1, or -1; every pair
 * runs against the same kf1 flags (the raw per-pair results, before CreateNewMapPoints drops the
 * features an earlier neighbour triangulated).  F12_out (n_pairs x 9, row-major), nmatches
 * (n_pairs).  Camera and scale pyramid from the context's configuration. */
int mmt_search_for_triangulation(mmt_ctx* ctx, const mmt_sft_keyframe* kf1, int n_pairs,
                                 const mmt_sft_keyframe* kf2, int32_t* match12_out,
                                 float* F12_out, int* nmatches);

/* Counters of the vocabulary path (tests): BoW conversions of frames, TrackReferenceKeyFrame calls
 * and successes, Relocalization calls and successes, candidate keyframes, PnPsolver poses,
 * SearchByProjection(F, KF) rounds, triangulated points, SearchForTriangulation matches, database
 * insertions. */
typedef struct mmt_bow_counters {
  int64_t bow_frames, trk, trk_ok, reloc, reloc_ok, reloc_cands, pnp_found, sbp_rounds,
      triangulated, sft_matches, kfdb;
} mmt_bow_counters;
int mmt_bow_counters_read(mmt_ctx* ctx, mmt_bow_counters* out);

/* The tracker's map as flat arrays (no reference counterpart: the map invariant tests and the
 * map-graph parity against the CPU oracle read it).  Keyframes and map points are numbered in
 * creation order (the reference's mnId order).  sizes[7] (out): keyframes, map points,
 * observations, connections, ordered covisibles, children, keyframe map-point slots.  With
 * out == NULL only the sizes are written; otherwise every array must hold its size. */
typedef struct mmt_map_dump_arrays {
  int64_t* kf_i;          /* n_kf x 4: mnId, mnFrameId, isBad, parent (-1: none)             */
  float* kf_T;            /* n_kf x 16: Tcw                                                   */
  int32_t* kf_mps_start;  /* n_kf + 1: CSR offsets into kf_mps                                */
  int32_t* kf_mps;        /* slots: mvpMapPoints (map point number or -1)                     */
  float* pt_f;            /* n_pt x 5: world position, mfMinDistance, mfMaxDistance             */
  int32_t* pt_i;          /* n_pt x 5: isBad, nObs, mpRefKF, mnFirstKFid, mpReplaced (-1)     */
  int32_t* obs_start;     /* n_pt + 1: CSR offsets into obs_i / obs_f (mObservations)          */
  int32_t* obs_i;         /* n_obs x 3: keyframe, key index, key octave                        */
  float* obs_f;           /* n_obs x 4: key x, y, mvDepth, mvuRight                            */
  int32_t* conn;          /* n_conn x 3: keyframe, other, weight (mConnectedKeyFrameWeights)   */
  int32_t* ord;           /* n_ord x 3: keyframe, other, weight (mvpOrderedConnectedKeyFrames) */
  int32_t* child;         /* n_child x 2: keyframe, child (mspChildrens)                        */
} mmt_map_dump_arrays;
int mmt_map_dump(mmt_ctx* ctx, int32_t* sizes, const mmt_map_dump_arrays* out);

/* Visualisation hook (no reference counterpart; Tracking.cc:684-783 draws these into feat.png):
 * the static samples (mvSiftKeys, B2) and the object samples (mvObjKeys with vSemObjLabel, B1)
 * of the last frame the context tracked, xy as n x 2 floats.  Counts clipped to the caps. */
int mmt_frame_samples(mmt_ctx* ctx, float* static_xy, int static_cap, int* n_static,
                      float* obj_xy, int32_t* obj_label, int obj_cap, int* n_obj);

/* ---- Object front end probes: one stage of the per-frame object path run alone on host arrays.
 * W and H are arguments (not the context's configuration); maps are W x H row-major, flow maps
 * W x H x 2 floats, masks int32.  Sample outputs hold `cap` entries; entries the stage does not
 * write come back with all bytes 0xFF. */

/* A2 (Tracking.cc:447-465): cvtColor(RGB2GRAY) on the colour bytes and disparity -> depth,
 * depth = bf / (float)(d / 256.0), for nframes frames of npix pixels in one launch.  Pitches are
 * per frame, in elements of the array (bytes for bgr and gray); gray and depth are read-write:
 * their padding keeps the caller's bytes. */
int mmt_gray_depth(mmt_ctx* ctx, const uint8_t* bgr, size_t bgr_pitch, const uint16_t* disp256,
                   size_t disp_pitch, int npix, int nframes, float bf, uint8_t* gray,
                   size_t gray_pitch, float* depth, size_t depth_pitch);

/* B2 (Frame.cc:228-324): the static ORB keys kept through the flow, in key order:
 * mvSiftKeysTmp, mvCorres, mvFlowNext, mvSiftDepthTmp; *count = min(kept, cap).  Keys must lie
 * inside the image (the maps are read at the truncated key). */
int mmt_static_samples(mmt_ctx* ctx, const mmt_kp* kps, int n, const float* depth,
                       const float* flow, const int32_t* mask, int W, int H, int cap,
                       float* keys_out, float* corres_out, float* flow_out, float* depth_out,
                       int* count);

/* B1 (Frame.cc:188-217): the semi-dense object samples of every 4th row and column, row-major:
 * mvObjKeys, mvObjCorres, mvObjFlowNext, mvObjDepth, vSemObjLabel; *count = min(kept, cap). */
int mmt_object_samples(mmt_ctx* ctx, const float* depth, const float* flow, const int32_t* mask,
                       int W, int H, int cap, float* keys_out, float* corres_out, float* flow_out,
                       float* depth_out, int32_t* label_out, int* count);

/* B4 (Tracking.cc:487-578): the last frame's correspondences become the current frame's keys;
 * depth (static: -1 unless > 0) and depth and label (object: 0.1 and 0 outside the image) are read
 * at the std::round coordinates, inside meaning 0 < round(u) < W and 0 < round(v) < H. */
int mmt_sample_handoff(mmt_ctx* ctx, const float* last_corres, int ns, const float* last_obj_corres,
                       int no, const float* depth, const int32_t* mask, int W, int H,
                       float* skeys_out, float* sdepth_out, float* okeys_out, float* odepth_out,
                       int32_t* olabel_out, int* ns_out, int* no_out);

/* B6 + B7 statistics (GetSceneFlowObj, Tracking.cc:4007-4093, with Frame::UnprojectStereoObject,
 * Frame.cc:1118-1152; the Posi lists and the per-object counters of Tracking.cc:1396-1536; the
 * last-label counts of Tracking.cc:1573-1585).  Sample i has its current key, depth and label and
 * its last-frame ones.  obj_label_out n: vObjLabel after GetSceneFlowObj (-1, or -2 where the
 * reference leaves its initial value); members_out 16 x max(n, 1): label l's sample indices
 * ascending in row l (Posi); stats_out 16 x 8 words per label: cnt, bcnt (samples in the boundary
 * band), sfcnt (scene flow under 0.12), members, depth_sum (a float: the samples' current depths
 * added in index order), three unused; hist_out 16 x 16: [current label][last label] counts.
 * A current or last label above 15 sets *err_out and fails the call with MMT_EINVAL. */
typedef struct mmt_obj_group_problem {
  int n;
  const float* cur_keys;   /* n x 2 */
  const float* cur_depth;
  const int32_t* cur_label;
  const float* last_keys;  /* n x 2 */
  const float* last_depth;
  const int32_t* last_label;
  float Tcur[16], Tlast[16]; /* row-major Tcw of the current and the last frame */
  float fx, fy, cx, cy;
  int W, H;
} mmt_obj_group_problem;
int mmt_object_groups(mmt_ctx* ctx, const mmt_obj_group_problem* problem, int32_t* obj_label_out,
                      int32_t* members_out, int32_t* stats_out, int32_t* hist_out, int* err_out);

/* Stage timing with HIP events on the launch stream (no reference counterpart: measurement
 * hook for bench.py).  orb_ms sums the batched ORB launch sequences of the tracked chunks. */
typedef struct mmt_profile {
  double orb_ms;
  int64_t orb_launches;
  int64_t orb_frames;
} mmt_profile;
int mmt_profile_enable(mmt_ctx* ctx, int on);
int mmt_profile_read(mmt_ctx* ctx, mmt_profile* out, int reset);

/* Forget the sequence (Tracking::Reset). */
int mmt_reset(mmt_ctx* ctx);

/* Deferred object results (no reference counterpart; for callers that track one frame, or one
 * short chunk, per call).  By default every mmt_track_rgbd* call returns each frame with its own
 * object motions, which drains the object pipeline (PnP-RANSAC, PoseOptimizationFlow2 per object)
 * at the end of every call.  With on = 1 a call returns each frame's pose and map state at once,
 * and in the object fields of its results the motions of the frames whose object path has
 * finished, oldest first (res[i].objects_frame names the frame; -1: none yet): every frame's
 * motions arrive exactly once, in order, up to 17 frames later.  mmt_flush_objects finishes the
 * pipeline and returns the remaining records (res[k].objects_frame, n_objects and objs[k *
 * objs_cap ..] only), at most res_cap per call: *n = records written, 0 when none remain.
 * Turning the mode off flushes (and drops) the records still owed; mmt_reset drops them.  While
 * a flush has records left for a later mmt_flush_objects call, every mmt_track_rgbd* call returns
 * MMT_ESTATE (it would deliver newer frames' motions first).
 * MMT_EINVAL when the host object worker (MMT_OBJ_THREAD=1) is on. */
int mmt_set_deferred_objects(mmt_ctx* ctx, int on);
int mmt_flush_objects(mmt_ctx* ctx, mmt_frame_result* res, mmt_motion* objs, int objs_cap,
                      int res_cap, int* n);

/* ---- Stereo frames: keypoint depth from a rectified image pair ----------------------------------
 * Counters of Frame::ComputeStereoMatches (Frame.cc:849-1038), one per rejection stage (no
 * reference counterpart: they make every stage observable).  n_coarse = n_window_edge +
 * n_end_shift + n_delta + n_range + n_accepted. */
typedef struct mmt_stereo_counters {
  int32_t n_coarse;          /* left keys whose best Hamming distance is below thOrbDist = 75
                                (Frame.cc:949)                                              */
  int32_t n_window_edge;     /* skipped by the border test of Frame.cc:972, or because the first
                                shifted window would start left of column 0 (pinned, below) */
  int32_t n_end_shift;       /* best shift -5 or +5 (Frame.cc:991)                          */
  int32_t n_delta;           /* parabola offset outside [-1, 1] (Frame.cc:1001)             */
  int32_t n_range;           /* disparity outside [0, 200) (Frame.cc:1009; a NaN lands here) */
  int32_t n_clamped;         /* accepted with a disparity of 0, set to 0.01 (Frame.cc:1011-1015) */
  int32_t n_accepted;        /* vDistIdx.size()                                             */
  int32_t n_median_removed;  /* cleared by the median filter (Frame.cc:1027-1037)           */
  int32_t median;            /* vDistIdx[size / 2].first (-1: no accepted key)              */
  float th_dist;             /* thDist = 1.5f * 1.4f * median (0: no accepted key)          */
} mmt_stereo_counters;

/* Frame::ComputeStereoMatches (Frame.cc:849-1038; this fork: minD = 0, maxD = 200 pixels, the
 * vDescIndex output) on caller-supplied keys.  left / right: 8-bit gray images of the context's
 * size (host pointers, row stride `stride`); both pyramids are built with the extractor's pyramid
 * stage (ORBextractor::ComputePyramid, ORBextractor.cc:1111-1136; no FAST), since the 11 x 11
 * correlation windows are read from the unblurred level of the left key (Frame.cc:960, 977).
 * kps / desc (n x 32) of both sides as the extractor writes them; n <= 16384 per side.
 * Outputs (n_left each): uR = mvuRight and depth = mvDepth (-1 without a match), right_idx =
 * vDescIndex (Frame.cc:943-944: the best right key unless it is key 0, which is never reported;
 * -1 again when the median filter clears the match); optional best_dist = the coarse search's
 * bestDist (100 when no candidate is closer, -1 when the key's row lists no right key) and sad =
 * the window search's bestDist (-1 where it is not reached).  Camera.bf from the configuration.
 * Pinned where the reference is undefined: without an accepted match nothing is cleared (the
 * reference reads an empty vector, Frame.cc:1024); a right key closer than 10 level pixels to the
 * left border (OpenCV would throw in colRange, Frame.cc:977) is skipped like Frame.cc:972.
 * MMT_EINVAL before any launch: config.max_batch < 2 (the device pyramid is frame-major per batch
 * slot, and a pair needs two slots), an octave outside the pyramid, a left key whose 11 x 11 window
 * leaves its level or whose row (int)y leaves the image, a right key whose row range floor(y - r)
 * .. ceil(y + r) (Frame.cc:873-878) leaves [0, rows). */
int mmt_stereo_matches(mmt_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h,
                       int stride, int n_left, const mmt_kp* kps_left, const uint8_t* desc_left,
                       int n_right, const mmt_kp* kps_right, const uint8_t* desc_right, float* uR,
                       float* depth, int32_t* right_idx, int32_t* best_dist, int32_t* sad,
                       mmt_stereo_counters* counters);

/* The stereo Frame constructor (Frame.cc:79-159) as System::TrackStereo -> Tracking::
 * GrabImageStereo reaches it: both gray images extracted as one batch of two (replacing the two
 * ExtractORB threads of Frame.cc:96-99), vSemLabel[i] = mask(int(y), int(x)) (Frame.cc:116-124;
 * mask: optional w x h int32, rows packed; sem_label is written only with a mask), mvKeysUn ==
 * mvKeys (no distortion), then ComputeStereoMatches against the two pyramids of the batch in
 * place.  kps / desc: the left keys, level-major and bit-identical to mmt_orb_extract(left);
 * kps_right / desc_right: the right keys.  *n / *n_right receive the counts; MMT_ENOSPC, as
 * mmt_orb_extract, when cap (the slots of kps, desc, uR, depth, right_idx, sem_label) or cap_right
 * is short of its count (known once the extraction has run; nothing is matched or copied then).
 * Without a left key (the early return of Frame.cc:103) the left outputs are empty and *n_right is
 * still reported.  MMT_EINVAL before any launch: config.max_batch < 2, an image size other than
 * the configuration's, mmt_orb_capacity() above 16384. */
int mmt_stereo_frame(mmt_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h,
                     int stride, const int32_t* mask, mmt_kp* kps, uint8_t* desc, int cap, int* n,
                     mmt_kp* kps_right, uint8_t* desc_right, int cap_right, int* n_right,
                     float* uR, float* depth, int32_t* right_idx, int32_t* sem_label,
                     mmt_stereo_counters* counters);

/* ---- Loop detection: keyframe database scores and loop candidates --------------------------------
 * LoopClosing::DetectLoop (LoopClosing.cc:105-231) and KeyFrameDatabase::DetectLoopCandidates
 * (KeyFrameDatabase.cc:76-197).  The context keeps every keyframe's BoW vector on the device; one
 * kernel launch scores a stored vector against all of them (common words, first common word, the
 * raw DBoW2 sum, added in word order: bit-identical to Vocabulary::score's loop), and the
 * order-dependent rest runs on the host as the reference writes it.  The tracker does not call
 * any of this.
 *
 * Most words of one stored vector; more is MMT_EINVAL (the query is staged in LDS: 12 bytes per
 * word, 96 KiB at the bound, of the CU's 160 KiB). */
#define MMT_LOOP_MAX_WORDS 8192

/* DBoW2::BowVector: n (word, value) pairs, word strictly ascending. */
typedef struct mmt_bow_vector {
  int n;
  const uint32_t* word;
  const double* value;
} mmt_bow_vector;

/* The covisibility graph the detection reads, indexed by keyframe id (mnId), 0 .. n_kf-1.  The two
 * lists differ in the reference: UpdateConnections keeps every keyframe that shares a map point
 * in mConnectedKeyFrameWeights and only those at or above the threshold in the ordered list
 * (KeyFrame.cc:289-367). */
typedef struct mmt_covis_graph {
  int n_kf;
  const int32_t* ordered_start;    /* n_kf + 1 */
  const int32_t* ordered;          /* mvpOrderedConnectedKeyFrames, weight descending:
                                      GetVectorCovisibleKeyFrames; its first 10 =
                                      GetBestCovisibilityKeyFrames(10) */
  const int32_t* conn_start;       /* n_kf + 1 */
  const int32_t* conn;             /* keys of mConnectedKeyFrameWeights = GetConnectedKeyFrames
                                      (a set; any order) */
  const uint8_t* bad;              /* isBad() */
} mmt_covis_graph;

typedef struct mmt_loop_result {
  int32_t ran;           /* 0: the early exit (mnId < mLastLoopKFid + 10), nothing was scored   */
  float min_score;       /* minScore over the non-bad covisible keyframes (1 without one)      */
  int32_t n_candidates;  /* vpCandidateKFs.size()                                               */
  int32_t n_enough;      /* mvpEnoughConsistentCandidates.size()                                */
  int32_t n_groups;      /* mvConsistentGroups.size() after the call                            */
} mmt_loop_result;

typedef struct mmt_loop_store_stats {
  int32_t n_stored;        /* vectors on the device                                            */
  int32_t n_members;       /* keyframes in the database                                        */
  int64_t word_capacity;   /* elements the device word array holds                             */
  int64_t value_capacity;  /* elements the device value array holds                            */
  int32_t word_grown;      /* times the word array was reallocated and copied                  */
  int32_t value_grown;     /* the same for the value array                                     */
} mmt_loop_store_stats;

/* Every call below returns MMT_EINVAL for an unknown keyframe id, an id outside the graph, a
 * vector that is not strictly ascending or too long, and an output buffer that is too small.
 *
 * mmt_loop_reset: empties the store, the database and the consistency groups; scoring is the
 *   vocabulary's field (0: L1, 1: L2; TemplatedVocabulary has no other that Vocabulary::score
 *   implements here).
 * mmt_loop_set_bow: KeyFrame::ComputeBoW's mBowVec onto the device, once per keyframe id (a second
 *   call for the same id is MMT_EINVAL; a stored vector never changes).
 * mmt_loop_db_add / _erase: KeyFrameDatabase::add / erase.  A member is added once (a second add
 *   is MMT_EINVAL); erasing a non-member does nothing.  The vector stays stored after an erase, as
 *   the keyframe keeps its mBowVec: minScore still reads it.
 * mmt_loop_scores (probe): the kernel's outputs for every stored vector against kf_id's, in
 *   storage order, with the finished double score (Vocabulary::score) and the keyframe ids.
 * mmt_detect_loop_candidates: DetectLoopCandidates(kf_id, min_score) in the reference's order; the
 *   database and the groups are not touched.
 * mmt_detect_loop: DetectLoop for keyframe kf_id (not yet a database member) with mLastLoopKFid =
 *   last_loop_kf_id and mnCovisibilityConsistencyTh = consistency_th (the reference: 3).  cand_out
 *   receives vpCandidateKFs, enough_out mvpEnoughConsistentCandidates (cap entries each); the
 *   keyframe is added to the database as the reference does on every path.  The reference's
 *   DetectLoop returns false in this fork whatever the list holds (LoopClosing.cc:225); acting on
 *   result->n_enough > 0 is the caller's business.  A non-bad covisible keyframe with no stored
 *   vector is MMT_EINVAL.  On an error nothing has changed.
 * mmt_loop_groups_read: mvConsistentGroups as a CSR of ascending member ids (group_start:
 *   n_groups + 1 entries) plus the consistency counters.
 * One kernel launch and one read-back (16 bytes per stored vector) per scores / candidates /
 * detect call; nothing but the slot index of kf_id goes up. */
int mmt_loop_reset(mmt_ctx* ctx, int scoring);
int mmt_loop_set_bow(mmt_ctx* ctx, int32_t kf_id, const mmt_bow_vector* v);
int mmt_loop_db_add(mmt_ctx* ctx, int32_t kf_id);
int mmt_loop_db_erase(mmt_ctx* ctx, int32_t kf_id);
int mmt_loop_scores(mmt_ctx* ctx, int32_t kf_id, int32_t* common, int32_t* first, double* sum,
                    double* score, int32_t* ids, int cap, int* n_out);
int mmt_detect_loop_candidates(mmt_ctx* ctx, int32_t kf_id, float min_score,
                               const mmt_covis_graph* graph, int32_t* cand_out, int cap,
                               int* n_out);
int mmt_detect_loop(mmt_ctx* ctx, int32_t kf_id, int32_t last_loop_kf_id, int consistency_th,
                    const mmt_covis_graph* graph, mmt_loop_result* result, int32_t* cand_out,
                    int32_t* enough_out, int cap);
int mmt_loop_groups_read(mmt_ctx* ctx, int32_t* group_start, int32_t* members, int32_t* counters,
                         int cap_groups, int cap_members, int* n_groups, int* n_members);
int mmt_loop_stats(mmt_ctx* ctx, mmt_loop_store_stats* out);

/* Upper bound on keypoints per frame: the sum over levels of max(quota, 4 * nIni) + 8 slots, where
 * DistributeOctTree keeps at most max(quota + 2, 4 * nIni) keys. */
int mmt_orb_capacity(const mmt_ctx* ctx);

/* ---- Debug and test hooks: not part of the stable interface, no reference counterpart ---- */

/* Test hook: OR `flags` into the ORB device error word (as a tripped kernel guard would). */
int mmt_debug_orb_raise(mmt_ctx* ctx, int flags);

/* Debug: copy an intermediate device buffer of the last ORB run (frame 0..max_batch-1) to the
 * host.  what: 0 pyramid, 1 blurred pyramid (both level-major, unpadded), 2 FAST per-cell
 * counts (int), 3 FAST candidate keys (packed u32), 4 octree output keys (packed u32),
 * 5 octree per-level counts (int), 6 device error flags (int).  Returns bytes written or <0. */
long mmt_debug_fetch(mmt_ctx* ctx, int what, int frame, void* out, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* MMT_H */
