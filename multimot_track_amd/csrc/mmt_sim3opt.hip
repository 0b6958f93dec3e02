// multimot_track_amd/csrc/mmt_sim3opt.hip -- Optimizer::OptimizeSim3 (reference
// src/Optimizer.cc:3934-4129) for a batch of loop candidates: LoopClosing::ComputeSim3 calls it on
// every candidate whose Sim3Solver round returned a similarity (LoopClosing.cc:322-341).
//
//   k_sim3_opt   one workgroup per problem, the whole call in one launch: both optimisation rounds
//                (g2o's Levenberg-Marquardt on the one free VertexSim3Expmap), the removal of the bad
//                pairs between them, the final inlier test and the results
//   host         argument checks, one staging block up, one block down
//
// Each correspondence carries two edges with fixed points: e12 = obs1 - cam_map1(project(S12 X2c))
// and e21 = obs2 - cam_map2(project(S12^-1 X1c)) (Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h),
// both under a Huber kernel of delta sqrtf(th2).  Neither edge type has an analytic Jacobian, so
// g2o differentiates numerically (core/base_binary_edge.hpp:131-205): column d is
// (e(oplus(+1e-9 e_d)) - e(oplus(-1e-9 e_d))) / 2e-9.  The 14 stepped estimates depend on the vertex
// only, so 15 lanes build them once per linearisation, each as the rows of (s R | t) and of its
// inverse, and every thread maps its correspondences through the 15 of them.  A trial evaluates
// errors and robust chi2 alone (one more transform); the 36 sums of a linearisation (28 of H's
// upper triangle, 7 of b, the robust chi2) meet in a fixed order (block_sum_tile), so a problem
// computes the same bits whatever else is in the batch.  The 7 x 7 LDLT runs on one lane.
//
// An edge keeps the error of the last computeActiveErrors, i.e. of the last trial's state: after a
// rejected trial g2o pops the vertex, not the edges' errors.  The inlier tests read those errors,
// so they evaluate the pairs at the last trial's transform.
//
// Arithmetic: double throughout (float inputs promoted on load), no FMA contraction.  The estimate
// is g2o::Sim3's (unnormalised Eigen quaternion, t, s); the maps go through its (s R | t) rows, which
// differs from s * (q * x) + t in rounding only.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "mmt_devbuf.h"
#include "mmt_devmath.h"
#include "mmt_internal.h"
#include "mmt_lmstep.h"
#include "mmt_sim3opt.h"

namespace mmt {
namespace {

constexpr int kSoSums = 36;    // [0] robust chi2, [1..28] H's upper triangle by rows, [29..35] b
constexpr int kSoStride = 37;  // odd row stride of the reduction tile
constexpr int kSoWaves = kSim3OptThreads / 64;
constexpr int kSoTrial = 15;   // transform slots: 0 the estimate, 1 + 2d / 2 + 2d its steps of
                               // +1e-9 / -1e-9 along d, 15 the trial
constexpr double kSoDelta = 1e-9;

struct DSim3 {  // g2o::Sim3
  DQuat q;
  double t[3];
  double s;
};

// Sim3(const Vector7d& update), sim3.h:70-142: (omega, upsilon, sigma), eps 1e-5
__device__ inline DSim3 sim3_exp(const double (&u)[7]) {
  const double o0 = u[0], o1 = u[1], o2 = u[2], sigma = u[6];
  const double theta = sqrt(o0 * o0 + o1 * o1 + o2 * o2);
  const double O[3][3] = {{0, -o2, o1}, {o2, 0, -o0}, {-o1, o0, 0}};
  double O2[3][3];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) O2[r][c] = O[r][0] * O[0][c] + O[r][1] * O[1][c] + O[r][2] * O[2][c];
  const double s = exp(sigma);
  const double eps = 0.00001;
  double A, B, C, ra, rb;  // R = I + ra Omega + rb Omega^2
  if (fabs(sigma) < eps) {
    C = 1;
    if (theta < eps) {
      A = 1. / 2.;
      B = 1. / 6.;
      ra = 1;
      rb = 1;
    } else {
      double st, ct;
      sincos(theta, &st, &ct);
      const double theta2 = theta * theta;
      A = (1 - ct) / theta2;
      B = (theta - st) / (theta2 * theta);
      ra = st / theta;
      rb = (1 - ct) / (theta * theta);
    }
  } else {
    C = (s - 1) / sigma;
    if (theta < eps) {
      const double sigma2 = sigma * sigma;
      A = ((sigma - 1) * s + 1) / sigma2;
      B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
      ra = 1;
      rb = 1;
    } else {
      double st, ct;
      sincos(theta, &st, &ct);
      ra = st / theta;
      rb = (1 - ct) / (theta * theta);
      const double a = s * st, b = s * ct;
      const double theta2 = theta * theta, sigma2 = sigma * sigma;
      const double c = theta2 + sigma2;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
    }
  }
  double R[3][3], W[3][3];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const double I = r == c ? 1.0 : 0.0;
      R[r][c] = (I + ra * O[r][c]) + rb * O2[r][c];
      W[r][c] = (A * O[r][c] + B * O2[r][c]) + C * I;
    }
  DSim3 S;
  S.q = dq_from_R(R);  // Quaterniond(R), not normalised
  S.s = s;
#pragma unroll
  for (int r = 0; r < 3; r++) S.t[r] = W[r][0] * u[3] + W[r][1] * u[4] + W[r][2] * u[5];
  return S;
}

__device__ inline DSim3 sim3_mul(const DSim3& a, const DSim3& b) {  // Sim3::operator*
  DSim3 r;
  r.q = dq_mul(a.q, b.q);
  double x, y, z;
  dq_rotate(a.q, b.t[0], b.t[1], b.t[2], x, y, z);
  r.t[0] = a.s * x + a.t[0];
  r.t[1] = a.s * y + a.t[1];
  r.t[2] = a.s * z + a.t[2];
  r.s = a.s * b.s;
  return r;
}

__device__ inline DSim3 sim3_inverse(const DSim3& a) {  // Sim3::inverse
  DSim3 r;
  r.q = DQuat{-a.q.x, -a.q.y, -a.q.z, a.q.w};
  const double m = -1. / a.s;
  dq_rotate(r.q, m * a.t[0], m * a.t[1], m * a.t[2], r.t[0], r.t[1], r.t[2]);
  r.s = 1. / a.s;
  return r;
}

// VertexSim3Expmap::oplusImpl
__device__ inline DSim3 sim3_oplus(const DSim3& S, double (&u)[7], int fix_scale) {
  if (fix_scale) u[6] = 0;
  return sim3_mul(sim3_exp(u), S);
}

// rows of (s R | t) into T[0..12) and of the inverse's into T[12..24)
__device__ inline void sim3_rows(const DSim3& S, double* T) {
  double R[3][3];
  dq_to_R(S.q, R);
#pragma unroll
  for (int r = 0; r < 3; r++) {
#pragma unroll
    for (int c = 0; c < 3; c++) T[4 * r + c] = S.s * R[r][c];
    T[4 * r + 3] = S.t[r];
  }
  const DSim3 I = sim3_inverse(S);
  dq_to_R(I.q, R);
#pragma unroll
  for (int r = 0; r < 3; r++) {
#pragma unroll
    for (int c = 0; c < 3; c++) T[12 + 4 * r + c] = I.s * R[r][c];
    T[12 + 4 * r + 3] = I.t[r];
  }
}

struct SoCam {
  double fx, fy, cx, cy;
};

struct SoPair {  // a correspondence, promoted
  double X1[3], X2[3], o1[2], o2[2], w1, w2;
};

// obs - cam_map(project(T X)), T 3 x 4 rows; no depth test (a zero depth gives a non-finite error)
__device__ __forceinline__ void so_err(const double* T, const double (&X)[3], const double (&o)[2],
                                       const SoCam& K, double& e0, double& e1) {
  const double x = ((T[0] * X[0] + T[1] * X[1]) + T[2] * X[2]) + T[3];
  const double y = ((T[4] * X[0] + T[5] * X[1]) + T[6] * X[2]) + T[7];
  const double z = ((T[8] * X[0] + T[9] * X[1]) + T[10] * X[2]) + T[11];
  e0 = o[0] - ((x / z) * K.fx + K.cx);
  e1 = o[1] - ((y / z) * K.fy + K.cy);
}

// BaseEdge::chi2 with the information w I
__device__ __forceinline__ double so_chi2(double e0, double e1, double w) {
  return e0 * (w * e0) + e1 * (w * e1);
}

// RobustKernelHuber::robustify
__device__ __forceinline__ void so_huber(double e, double delta, double dsqr, double& r0,
                                         double& r1) {
  if (e <= dsqr) {
    r0 = e;
    r1 = 1.;
  } else {
    const double sqrte = sqrt(e);
    r0 = 2 * sqrte * delta - dsqr;
    r1 = delta / sqrte;
  }
}

struct SoSmem {
  double tile[kSoWaves * 64 * kSoStride];
  double part[kSoWaves * kSoSums];
  double H[kSoSums];     // the sums of the current estimate's linearisation
  double T[kSoTrial + 1][24];
  double red[kSoWaves * 32];
  double one[32];
  DSim3 cur, trial;
  double x[7];
  int ok2;
  // the LDLT's workspace (one lane, indexed at run time)
  double A[7][7], L[7][7], D[7], y[7];
  int perm[7];
};

// Eigen::LDLT<MatrixXd> of H + lambda I with diagonal pivoting (LinearSolverDense), on one lane:
// sm.x receives the solution when the factorisation is positive (LDLT::isPositive()), and keeps its
// values otherwise (g2o's stale increment).  (The 6 x 6 solves of mmt_lm.hip, ldlt6_packed, are
// unpivoted and unrolled in registers instead.)
__device__ __noinline__ void so_solve(SoSmem& sm, const double* Hc, double lam) {
  {
    int k = 1;
  #pragma unroll 1
  for (int a = 0; a < 7; a++)
    #pragma unroll 1
  for (int b = a; b < 7; b++) {
        const double h = Hc[k++];
        sm.A[a][b] = sm.A[b][a] = a == b ? h + lam : h;
      }
  }
#pragma unroll 1
  for (int r = 0; r < 7; r++) {
    sm.perm[r] = r;
  #pragma unroll 1
  for (int c = 0; c < 7; c++) sm.L[r][c] = 0.0;
  }
  bool positive = true;
#pragma unroll 1
  for (int k = 0; k < 7; k++) {
    int p = k;
    double best = fabs(sm.A[k][k]);
  #pragma unroll 1
  for (int i = k + 1; i < 7; i++)
      if (fabs(sm.A[i][i]) > best) {
        best = fabs(sm.A[i][i]);
        p = i;
      }
    if (p != k) {
    #pragma unroll 1
  for (int c = 0; c < 7; c++) {
        const double t = sm.A[k][c];
        sm.A[k][c] = sm.A[p][c];
        sm.A[p][c] = t;
      }
    #pragma unroll 1
  for (int r = 0; r < 7; r++) {
        const double t = sm.A[r][k];
        sm.A[r][k] = sm.A[r][p];
        sm.A[r][p] = t;
      }
    #pragma unroll 1
  for (int c = 0; c < k; c++) {
        const double t = sm.L[k][c];
        sm.L[k][c] = sm.L[p][c];
        sm.L[p][c] = t;
      }
      const int t = sm.perm[k];
      sm.perm[k] = sm.perm[p];
      sm.perm[p] = t;
    }
    double d = sm.A[k][k];
  #pragma unroll 1
  for (int c = 0; c < k; c++) d -= sm.L[k][c] * sm.L[k][c] * sm.D[c];
    sm.D[k] = d;
    if (d < 0) positive = false;
  #pragma unroll 1
  for (int i = k + 1; i < 7; i++) {
      double s = sm.A[i][k];
    #pragma unroll 1
  for (int c = 0; c < k; c++) s -= sm.L[i][c] * sm.L[k][c] * sm.D[c];
      sm.L[i][k] = (d != 0) ? s / d : 0.0;
    }
    sm.L[k][k] = 1.0;
  }
  sm.ok2 = positive ? 1 : 0;
  if (!positive) return;
#pragma unroll 1
  for (int i = 0; i < 7; i++) sm.y[i] = Hc[29 + sm.perm[i]];
#pragma unroll 1
  for (int i = 0; i < 7; i++)
  #pragma unroll 1
  for (int c = 0; c < i; c++) sm.y[i] -= sm.L[i][c] * sm.y[c];
#pragma unroll 1
  for (int i = 0; i < 7; i++) sm.y[i] = (sm.D[i] != 0) ? sm.y[i] / sm.D[i] : 0.0;
#pragma unroll 1
  for (int i = 6; i >= 0; i--)
  #pragma unroll 1
  for (int r = i + 1; r < 7; r++) sm.y[i] -= sm.L[r][i] * sm.y[r];
#pragma unroll 1
  for (int i = 0; i < 7; i++) sm.x[sm.perm[i]] = sm.y[i];
}

}  // namespace

__global__ __launch_bounds__(kSim3OptThreads) void k_sim3_opt(Sim3OptArgs a) {
  __shared__ SoSmem sm;
  const Sim3OptDev& P = a.prob[blockIdx.x];
  const int n = P.n;
  if (n <= 0) return;  // the host has written this problem's result
  const int tid = threadIdx.x;
  const size_t o = (size_t)P.pt_off;
  const float* X1c = a.X1c + 3 * o;
  const float* X2c = a.X2c + 3 * o;
  const float* obs1 = a.obs1 + 2 * o;
  const float* obs2 = a.obs2 + 2 * o;
  const float* w1 = a.w1 + o;
  const float* w2 = a.w2 + o;
  double* chi2 = a.chi2 + 2 * o;
  uint8_t* kept = a.kept + o;
  const SoCam K1 = {(double)P.fx1, (double)P.fy1, (double)P.cx1, (double)P.cy1};
  const SoCam K2 = {(double)P.fx2, (double)P.fy2, (double)P.cx2, (double)P.cy2};
  const int fix_scale = P.fix_scale;
  const double th2 = (double)P.th2;
  const double delta = (double)sqrtf(P.th2);  // const float deltaHuber = sqrt(th2)
  const double dsqr = delta * delta;          // RobustKernelHuber::setDelta

  auto load = [&](int i) {
    SoPair p;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      p.X1[k] = (double)X1c[3 * (size_t)i + k];
      p.X2[k] = (double)X2c[3 * (size_t)i + k];
    }
#pragma unroll
    for (int k = 0; k < 2; k++) {
      p.o1[k] = (double)obs1[2 * (size_t)i + k];
      p.o2[k] = (double)obs2[2 * (size_t)i + k];
    }
    p.w1 = (double)w1[i];
    p.w2 = (double)w2[i];
    return p;
  };
  // one edge's terms of the system: numeric Jacobian through the 14 stepped transforms (OFF 0:
  // e12 through the transform, OFF 12: e21 through its inverse), then constructQuadraticForm
  auto edge_terms = [&](int OFF, const double (&X)[3], const double (&ob)[2], const SoCam& K,
                        double w, double (&v)[kSoSums]) {
    double e0, e1, J0[7] = {0, 0, 0, 0, 0, 0, 0}, J1[7] = {0, 0, 0, 0, 0, 0, 0};
    so_err(sm.T[0] + OFF, X, ob, K, e0, e1);
    const double scalar = 1.0 / (2 * kSoDelta);
    // a rolled loop: unrolled, the compiler keeps the rows of all 15 transforms (720 registers)
    // live across the pair loop and spills.  The column lands in J by selects, so J stays in
    // registers.
#pragma unroll 1
    for (int d = 0; d < 7; d++) {
      double p0, p1, m0, m1;
      so_err(sm.T[1 + 2 * d] + OFF, X, ob, K, p0, p1);
      so_err(sm.T[2 + 2 * d] + OFF, X, ob, K, m0, m1);
      const double j0 = scalar * (p0 - m0), j1 = scalar * (p1 - m1);
#pragma unroll
      for (int k = 0; k < 7; k++) {
        J0[k] = k == d ? j0 : J0[k];
        J1[k] = k == d ? j1 : J1[k];
      }
    }
    double r0, r1;
    so_huber(so_chi2(e0, e1, w), delta, dsqr, r0, r1);
    v[0] += r0;
    const double wo = r1 * w;  // robustInformation
    const double or0 = -(w * e0) * r1, or1 = -(w * e1) * r1;
    int k = 1;
#pragma unroll
    for (int p = 0; p < 7; p++)
#pragma unroll
      for (int q = p; q < 7; q++) v[k++] += (J0[p] * wo) * J0[q] + (J1[p] * wo) * J1[q];
#pragma unroll
    for (int p = 0; p < 7; p++) v[29 + p] += J0[p] * or0 + J1[p] * or1;
  };
  // computeActiveErrors + buildSystem at sm.cur: the 36 sums into out (LDS)
  auto full = [&](double* out) {
    if (tid <= 14) {
      DSim3 S = sm.cur;
      if (tid > 0) {
        const int d = (tid - 1) >> 1;
        const double h = (tid & 1) ? kSoDelta : -kSoDelta;
        double u[7];
#pragma unroll
        for (int k = 0; k < 7; k++) u[k] = k == d ? h : 0.0;
        S = sim3_oplus(S, u, fix_scale);
      }
      sim3_rows(S, sm.T[tid]);
    }
    __syncthreads();
    double v[kSoSums];
#pragma unroll
    for (int k = 0; k < kSoSums; k++) v[k] = 0;
    for (int i = tid; i < n; i += kSim3OptThreads) {
      if (!kept[i]) continue;
      const SoPair p = load(i);
      edge_terms(0, p.X2, p.o1, K1, p.w1, v);
      edge_terms(12, p.X1, p.o2, K2, p.w2, v);
    }
    double* row = tile_row<kSoStride>(sm.tile);
#pragma unroll
    for (int k = 0; k < kSoSums; k++) row[k] = v[k];
    block_sum_tile<kSoSums, kSoStride>(sm.tile, sm.part, out, kSoWaves);
  };
  // computeActiveErrors + activeRobustChi2 at the trial transform (slot kSoTrial)
  auto light = [&]() {
    double c[1] = {0};
    for (int i = tid; i < n; i += kSim3OptThreads) {
      if (!kept[i]) continue;
      const SoPair p = load(i);
      double e0, e1, r0, r1;
      so_err(sm.T[kSoTrial], p.X2, p.o1, K1, e0, e1);
      so_huber(so_chi2(e0, e1, p.w1), delta, dsqr, r0, r1);
      c[0] += r0;
      so_err(sm.T[kSoTrial] + 12, p.X1, p.o2, K2, e0, e1);
      so_huber(so_chi2(e0, e1, p.w2), delta, dsqr, r0, r1);
      c[0] += r0;
    }
    block_sum<1>(c, sm.red, sm.one, kSoWaves);
    const double s = sm.one[0];
    __syncthreads();  // sm.one is rewritten by the next sum
    return s;
  };
  // the inlier test (Optimizer.cc:4073-4091, :4107-4122) on the edges' last computed errors, those
  // of the last trial (slot kSoTrial).  FINAL: a pair stays only if it also survived round 1; every
  // pair's chi2 is reported at this state.  Returns the number of pairs that fail / that stay.
  auto test = [&](bool FINAL) {
    double c[1] = {0};
    for (int i = tid; i < n; i += kSim3OptThreads) {
      const SoPair p = load(i);
      double e0, e1;
      so_err(sm.T[kSoTrial], p.X2, p.o1, K1, e0, e1);
      const double c12 = so_chi2(e0, e1, p.w1);
      so_err(sm.T[kSoTrial] + 12, p.X1, p.o2, K2, e0, e1);
      const double c21 = so_chi2(e0, e1, p.w2);
      chi2[2 * (size_t)i] = c12;
      chi2[2 * (size_t)i + 1] = c21;
      const bool bad = c12 > th2 || c21 > th2;
      if (FINAL) {
        const bool in = kept[i] && !bad;
        kept[i] = in ? 1 : 0;
        c[0] += in ? 1.0 : 0.0;
      } else {
        kept[i] = bad ? 0 : 1;
        c[0] += bad ? 1.0 : 0.0;
      }
    }
    block_sum<1>(c, sm.red, sm.one, kSoWaves);
    const int cnt = (int)sm.one[0];
    __syncthreads();
    return cnt;
  };

  for (int i = tid; i < n; i += kSim3OptThreads) kept[i] = 1;
  if (tid == 0) {
    double R[3][3];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) R[r][c] = (double)P.R12[3 * r + c];
    sm.cur.q = dq_from_R(R);  // g2o::Sim3(R, t, s): Quaterniond(R)
    sm.cur.t[0] = (double)P.t12[0];
    sm.cur.t[1] = (double)P.t12[1];
    sm.cur.t[2] = (double)P.t12[2];
    sm.cur.s = (double)P.s12;
  }
  __syncthreads();

  int nBad = 0, nIn = 0, second = 0;
  int stats[4] = {0, 0, 0, 0};
  // One call site each for the three passes (the linearisation of an accepted trial's state is
  // deferred to the next trial's start, and skipped when the round ends there): inlined more
  // often, the kernel spills.
#pragma unroll 1
  for (int round = 0; round < 2; round++) {
    const int iterations = round == 0 ? 5 : (nBad > 0 ? 10 : 5);
    LMStep lm;
    bool relinearise = true, first = true, go = true;
    if (tid < 7) sm.x[tid] = 0;
#pragma unroll 1
    for (int iter = 0; iter < iterations && go; iter++) {
      double lastTrialChi = 0;
#pragma unroll 1
      for (int q = 0; q < 10; q++) {
        if (relinearise) {
          full(sm.H);  // computeActiveErrors + buildSystem at the current estimate
          relinearise = false;
          if (first) {
            double md = 0;
            int k = 1;
#pragma unroll
            for (int p = 0; p < 7; p++) {
              md = fmax(md, fabs(sm.H[k]));
              k += 7 - p;
            }
            lm.begin_round(sm.H[0], md);
            first = false;
          }
        }
        if (q == 0) lm.begin_iteration();
        const double lam = lm.lam;
        __syncthreads();  // everyone is done with the last trial's increment and transform
        if (tid == 0) {
          so_solve(sm, sm.H, lam);
          if (fix_scale) sm.x[6] = 0;  // oplusImpl writes through the solver's increment
          double u[7];
#pragma unroll
          for (int k = 0; k < 7; k++) u[k] = sm.x[k];
          sm.trial = sim3_oplus(sm.cur, u, fix_scale);
          sim3_rows(sm.trial, sm.T[kSoTrial]);
        }
        __syncthreads();
        lastTrialChi = light();
        double scale = 0;
#pragma unroll
        for (int k = 0; k < 7; k++) scale += sm.x[k] * (lam * sm.x[k] + sm.H[29 + k]);
        stats[2 + round]++;
        if (lm.trial<LMCube::kPow>(lastTrialChi, sm.ok2 != 0, scale)) {
          __syncthreads();
          if (tid == 0) sm.cur = sm.trial;
          __syncthreads();  // the next full() reads sm.cur on 15 lanes
          relinearise = true;
        }
        if (!lm.another_trial()) break;
      }
      stats[round]++;
      go = lm.end_iteration(iter, lastTrialChi);
    }
    const int cnt = test(round == 1);
    if (round == 0) {
      nBad = cnt;
      if (n - nBad < 10) break;  // Optimizer.cc:4099
      second = 1;
    } else {
      nIn = cnt;
    }
  }
  __syncthreads();
  if (tid == 0) {
    Sim3OptOut& O = a.out[blockIdx.x];
    O.n_inliers = nIn;
    O.n_bad = nBad;
    O.second_round = second;
    O.pad = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) O.stats[k] = stats[k];
    if (second) {
      double R[3][3];
      dq_to_R(sm.cur.q, R);
      O.s = sm.cur.s;
#pragma unroll
      for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) O.R[3 * r + c] = R[r][c];
        O.t[r] = sm.cur.t[r];
      }
    } else {  // g2oS12 is not written back
      O.s = (double)P.s12;
#pragma unroll
      for (int k = 0; k < 9; k++) O.R[k] = (double)P.R12[k];
#pragma unroll
      for (int k = 0; k < 3; k++) O.t[k] = (double)P.t12[k];
    }
  }
}

void launch_sim3_opt(const Sim3OptArgs& a, int n_problems, hipStream_t st) {
  if (n_problems <= 0) return;
  hipLaunchKernelGGL(k_sim3_opt, dim3(n_problems), dim3(kSim3OptThreads), 0, st, a);
  MMT_HIP(hipGetLastError());
}

void sim3_optimize_gpu(hipStream_t s, int n_problems, const mmt_sim3_opt_problem* problems,
                       mmt_sim3_opt_result* results) {
  if (n_problems < 0 || n_problems > kSim3OptMaxProblems)
    throw ArgError("OptimizeSim3: more than 64 problems in one call");
  size_t n_pts = 0;
  std::vector<Sim3OptDev> dev(std::max(n_problems, 1));
  for (int i = 0; i < n_problems; i++) {
    const mmt_sim3_opt_problem& pr = problems[i];
    const mmt_sim3_opt_result& r = results[i];
    if (pr.n < 0 || pr.n > kSim3OptMaxPairs) throw ArgError("OptimizeSim3: n outside [0, 16384]");
    if (pr.n > 0 && (!pr.X1c || !pr.X2c || !pr.obs1 || !pr.obs2 || !pr.inv_sigma2_1 ||
                     !pr.inv_sigma2_2 || !r.kept))
      throw ArgError("OptimizeSim3: null problem or result arrays");
    if (!(pr.th2 > 0) || !std::isfinite(pr.th2))
      throw ArgError("OptimizeSim3: th2 not positive and finite");
    bool finite = std::isfinite(pr.s12);
    for (int k = 0; k < 9; k++) finite = finite && std::isfinite(pr.R12[k]);
    for (int k = 0; k < 3; k++) finite = finite && std::isfinite(pr.t12[k]);
    if (!finite || !(pr.s12 > 0)) throw ArgError("OptimizeSim3: S12 not finite or s12 <= 0");
    Sim3OptDev& D = dev[i];
    memset(&D, 0, sizeof(D));
    D.n = pr.n;
    D.pt_off = (int)n_pts;
    D.fix_scale = pr.fix_scale ? 1 : 0;
    D.th2 = pr.th2;
    D.fx1 = pr.fx1; D.fy1 = pr.fy1; D.cx1 = pr.cx1; D.cy1 = pr.cy1;
    D.fx2 = pr.fx2; D.fy2 = pr.fy2; D.cx2 = pr.cx2; D.cy2 = pr.cy2;
    D.s12 = pr.s12;
    memcpy(D.R12, pr.R12, sizeof(D.R12));
    memcpy(D.t12, pr.t12, sizeof(D.t12));
    n_pts += (size_t)pr.n;
  }
  // n == 0 (and every problem before the download): nothing ran, 0 inliers, S12 is the input
  for (int i = 0; i < n_problems; i++) {
    const mmt_sim3_opt_problem& pr = problems[i];
    mmt_sim3_opt_result& r = results[i];
    r.n_inliers = r.n_bad = r.second_round = 0;
    memset(r.stats, 0, sizeof(r.stats));
    r.s = (double)pr.s12;
    for (int k = 0; k < 9; k++) r.R[k] = (double)pr.R12[k];
    for (int k = 0; k < 3; k++) r.t[k] = (double)pr.t12[k];
  }
  if (n_pts == 0) return;
  // one staging block up: the problem records, then the six float arrays of every problem
  const size_t o_dev = 0;
  const size_t o_f = al16(o_dev + sizeof(Sim3OptDev) * (size_t)n_problems);
  const size_t up_bytes = o_f + 4 * 12 * n_pts;
  std::vector<uint8_t> up(up_bytes);
  memcpy(up.data() + o_dev, dev.data(), sizeof(Sim3OptDev) * (size_t)n_problems);
  float* f = (float*)(up.data() + o_f);
  float* fX1 = f;
  float* fX2 = fX1 + 3 * n_pts;
  float* fo1 = fX2 + 3 * n_pts;
  float* fo2 = fo1 + 2 * n_pts;
  float* fw1 = fo2 + 2 * n_pts;
  float* fw2 = fw1 + n_pts;
  for (int i = 0; i < n_problems; i++) {
    const mmt_sim3_opt_problem& pr = problems[i];
    if (pr.n == 0) continue;
    const size_t o = (size_t)dev[i].pt_off, m = (size_t)pr.n;
    memcpy(fX1 + 3 * o, pr.X1c, 12 * m);
    memcpy(fX2 + 3 * o, pr.X2c, 12 * m);
    memcpy(fo1 + 2 * o, pr.obs1, 8 * m);
    memcpy(fo2 + 2 * o, pr.obs2, 8 * m);
    memcpy(fw1 + o, pr.inv_sigma2_1, 4 * m);
    memcpy(fw2 + o, pr.inv_sigma2_2, 4 * m);
  }
  // one block down: the result records, every pair's two chi2, every pair's flag
  const size_t o_out = 0;
  const size_t o_chi = al16(o_out + sizeof(Sim3OptOut) * (size_t)n_problems);
  const size_t o_kept = o_chi + 16 * n_pts;
  const size_t down_bytes = o_kept + n_pts;
  DevBuf<uint8_t> d_up(up_bytes), d_down(down_bytes);
  std::vector<uint8_t> down(down_bytes);
  d_up.up(up, s);
  Sim3OptArgs a;
  a.prob = (const Sim3OptDev*)(d_up.p + o_dev);
  const float* df = (const float*)(d_up.p + o_f);
  a.X1c = df;
  a.X2c = a.X1c + 3 * n_pts;
  a.obs1 = a.X2c + 3 * n_pts;
  a.obs2 = a.obs1 + 2 * n_pts;
  a.w1 = a.obs2 + 2 * n_pts;
  a.w2 = a.w1 + n_pts;
  a.out = (Sim3OptOut*)(d_down.p + o_out);
  a.chi2 = (double*)(d_down.p + o_chi);
  a.kept = d_down.p + o_kept;
  launch_sim3_opt(a, n_problems, s);
  d_down.down(down.data(), down_bytes, s);
  MMT_HIP(hipStreamSynchronize(s));
  const Sim3OptOut* out = (const Sim3OptOut*)(down.data() + o_out);
  const double* chi = (const double*)(down.data() + o_chi);
  for (int i = 0; i < n_problems; i++) {
    const mmt_sim3_opt_problem& pr = problems[i];
    if (pr.n == 0) continue;
    mmt_sim3_opt_result& r = results[i];
    const Sim3OptOut& O = out[i];
    const size_t o = (size_t)dev[i].pt_off;
    r.n_inliers = O.n_inliers;
    r.n_bad = O.n_bad;
    r.second_round = O.second_round;
    memcpy(r.stats, O.stats, sizeof(r.stats));
    r.s = O.s;
    memcpy(r.R, O.R, sizeof(r.R));
    memcpy(r.t, O.t, sizeof(r.t));
    memcpy(r.kept, down.data() + o_kept + o, (size_t)pr.n);
    if (r.chi2) memcpy(r.chi2, chi + 2 * o, 16 * (size_t)pr.n);
  }
}

}  // namespace mmt
