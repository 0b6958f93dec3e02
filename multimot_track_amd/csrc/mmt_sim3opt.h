// multimot_track_amd/csrc/mmt_sim3opt.h -- device records of the batched OptimizeSim3
// (LoopClosing's ComputeSim3 step 4; reference src/Optimizer.cc:3934-4129).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mmt.h"

namespace mmt {

constexpr int kSim3OptMaxProblems = 64;  // problems of one call
constexpr int kSim3OptMaxPairs = 16384;  // correspondences of one problem
constexpr int kSim3OptThreads = 256;     // k_sim3_opt's workgroup

struct Sim3OptDev {  // one problem of the batch
  int n;             // correspondences
  int pt_off;        // its first row in the batch's point arrays
  int fix_scale;
  float th2;
  float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;
  float s12, R12[9], t12[3];  // the start (gScm's constructor arguments)
  int pad;
};

struct Sim3OptOut {  // what the workgroup reports
  int n_inliers, n_bad, second_round, pad;
  int stats[4];      // iterations of round 1 / 2, trials of round 1 / 2
  double s, R[9], t[3];
};

struct Sim3OptArgs {
  const Sim3OptDev* prob;
  const float* X1c;  // every problem's pairs, n x 3 each
  const float* X2c;
  const float* obs1;  // n x 2
  const float* obs2;
  const float* w1;   // invSigma2 of the two keys
  const float* w2;
  Sim3OptOut* out;
  double* chi2;      // 2 per pair: e12 / e21 chi2() at the last tested state
  uint8_t* kept;     // 1 per pair
};

void launch_sim3_opt(const Sim3OptArgs& a, int n_problems, hipStream_t st);

// Optimizer::OptimizeSim3 for n_problems candidates (mmt_optimize_sim3's semantics, include/mmt.h;
// throws ArgError on bad arguments)
void sim3_optimize_gpu(hipStream_t s, int n_problems, const mmt_sim3_opt_problem* problems,
                       mmt_sim3_opt_result* results);

}  // namespace mmt
