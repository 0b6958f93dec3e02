// multimot_track_amd/csrc/mmt_sim3.h -- device records of the batched Sim3Solver (LoopClosing's
// ComputeSim3 step 2; reference src/Sim3Solver.cc).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mmt.h"

namespace mmt {

constexpr int kSim3MaxSolvers = 64;   // solvers of one call
constexpr int kSim3MaxIters = 300;    // hypotheses per solver and call
constexpr int kSim3ScoreThreads = 1024;  // k_sim3_score's workgroup

struct Sim3SolverDev {  // one solver of the batch
  int n;                // correspondences
  int pt_off;           // its first row in the batch's point arrays
  int hyp_off;          // its first hypothesis of this call
  int fix_scale;
  long long flag_off;   // its first byte in the flag array (hypothesis-major, n bytes each)
  float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;
};

struct Sim3Hyp {        // ComputeSim3's products for one minimal set
  float T12[12];        // rows of (s R | t)
  float T21[12];        // rows of (1/s R^T | -1/s R^T t)
  float R[9], t[3], s;
  int pad[3];
};

struct Sim3Args {
  const Sim3SolverDev* sol;
  const int* hsol;      // hypothesis -> solver
  const int* sub;       // n_hyp x 3 correspondence indices (the minimal sets)
  int n_hyp;
  const float* X1;      // mvX3Dc1 of every solver, n x 3 each
  const float* X2;
  const float* max_err1;  // mvnMaxError1 / 2 as the comparison reads them
  const float* max_err2;
  Sim3Hyp* hyp;
  uint8_t* flags;       // mvbInliersi of every hypothesis
  int* count;           // mnInliersi
};

void launch_sim3(const Sim3Args& a, hipStream_t st);

// Sim3Solver::SetRansacParameters + iterate(n_iterations) for n_solvers solvers
// (mmt_sim3solver_iterate's semantics, include/mmt.h; throws ArgError on bad arguments)
void sim3solver_iterate_gpu(hipStream_t s, int n_solvers, const mmt_sim3_problem* problems,
                            const int32_t* const* randi, const int32_t* n_draw_iters,
                            int n_iterations, mmt_sim3_state* states, mmt_sim3_result* results,
                            mmt_sim3_probe* probes);

}  // namespace mmt
