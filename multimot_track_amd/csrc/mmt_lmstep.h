// multimot_track_amd/csrc/mmt_lmstep.h -- g2o's Levenberg-Marquardt step policy as the
// pose (D1), flow (D2 / D3) and local-BA solvers run it: OptimizationAlgorithmLevenberg::solve (lambda
// init tau * max diagonal, rho with the 1e-3 scale term, the 2/3 - 1/3 lambda update, ni doubling,
// at most 10 trials per iteration) and the stops of ORB-SLAM2's SparseOptimizer::optimize ("Raul's"
// three iterations with under 0.1 % gain, and a last-trial chi2 above the previous iteration's).
// Plain C++: the state is a struct that D1's scratch kernel (k_pose_opt) keeps in registers and the
// BA chain keeps in device memory (BAState).  What only the caller knows stays with the caller: the
// solve, the stale-x rule's increment, swapping the pose or the buffers after an accepted trial.
// The two hot loops of mmt_lm.hip (flow_lm_body: D2 / D3, pose_opt_light: D1 up to 2048 edges)
// still write the same policy out by hand: they sit at the register ceiling, and calling this
// struct there cost 0.5-0.9 % of the bench.  A change here goes there too.
// The CPU checker has its own restatement (oracle/oracle_solve.h) and does not include this file.
#pragma once

#include <cfloat>
#include <cmath>

#if defined(__HIPCC__)
#define MMT_LM_HD __host__ __device__ __forceinline__
#else
#define MMT_LM_HD inline
#endif

namespace mmt {

// How alpha = 1 - (2 rho - 1)^3 forms its cube.  g2o calls pow(., 3), and so do the local BA and
// the CPU checker; D1 / D2 / D3 multiply twice.  On the device pow is the general routine, not two
// multiplies, so the two forms may differ in the last bit of lambda: each solver keeps the form it
// has always had.
enum class LMCube { kMul, kPow };

struct LMStep {
  double lam, ni;  // damping and its rejection factor
  double chk;      // the previous iteration's last trial chi2 (the chi2-increase stop)
  double cur, ini;  // chi2 of the current estimate, and at the iteration's start
  double rho;      // of the last trial
  int qmax;        // trials of this iteration
  int strikes;     // Raul's stop: consecutive iterations with under 0.1 % gain

  static MMT_LM_HD double lambda_init(double maxdiag) { return 1e-5 * maxdiag; }

  // chi: chi2 at the round's first linearisation; maxdiag: the largest diagonal entry of H
  MMT_LM_HD void begin_round(double chi, double maxdiag) {
    cur = chi;
    lam = lambda_init(maxdiag);
    ni = 2;
    chk = 0;
    strikes = 0;
  }

  MMT_LM_HD void begin_iteration() {
    ini = cur;
    qmax = 0;
  }

  // One trial's decision.  lastTrialChi: chi2 at the trial state; ok2: the linear solve succeeded
  // (otherwise the trial re-applied the stale increment and cannot be accepted); scale: the
  // increment's x^T (lambda x + b).  True when the trial is accepted (the caller then makes the
  // trial state the current one).
  template <LMCube CUBE>
  MMT_LM_HD bool trial(double lastTrialChi, bool ok2, double scale) {
    const double tempChi = ok2 ? lastTrialChi : DBL_MAX;
    scale += 1e-3;
    rho = (cur - tempChi) / scale;
    const bool accept = rho > 0 && std::isfinite(tempChi);
    if (accept) {
      const double t = 2 * rho - 1;
      double alpha = 1. - (CUBE == LMCube::kPow ? pow(t, 3) : t * t * t);
      alpha = fmin(alpha, 2. / 3.);
      lam = lam * fmax(1. / 3., alpha);
      ni = 2;
      cur = tempChi;
    } else {
      lam = lam * ni;
      ni = ni * 2;
    }
    qmax++;
    return accept;
  }

  MMT_LM_HD bool another_trial() const { return rho < 0 && qmax < 10; }

  // After the iteration's last trial; false stops the round.
  MMT_LM_HD bool end_iteration(int iter, double lastTrialChi) {
    bool ok = true;
    if (qmax == 10 || rho == 0) ok = false;
    if (ok) {
      if ((ini - cur) * 1e3 < ini)
        strikes++;
      else
        strikes = 0;
      if (strikes >= 3) ok = false;
    }
    if (chk < lastTrialChi && iter > 0) ok = false;
    chk = lastTrialChi;
    return ok;
  }
};

}  // namespace mmt
