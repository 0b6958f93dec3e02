// multimot_track_amd/csrc/mmt_sim3.hip -- Sim3Solver (reference src/Sim3Solver.cc) for a batch of
// solvers: LoopClosing::ComputeSim3 visits its candidate keyframes round-robin with iterate(5)
// each (LoopClosing.cc:287-340), so one call runs the hypotheses of every candidate's next round.
//
//   k_sim3_hyp    one lane per (solver, hypothesis): ComputeSim3 (Horn 1987) on the three gathered
//                 point pairs, Sim3Solver.cc:226-337
//   k_sim3_score  one workgroup per hypothesis: CheckInliers (:340-364), both projections per
//                 correspondence, a flag byte each and the count
//   host          SetRansacParameters (:114-138), the minimal sets from the caller's RandomInt
//                 draws, and iterate()'s loop (:140-207) replayed over the counts
//
// Arithmetic: float in the reference's operation order; what the reference leaves to OpenCV follows
// DESIGN.md section 2 (cv::Mat products summed in double and rounded to float, cv::eigen as a
// double cyclic Jacobi, cv::Rodrigues in double).

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "mmt_devbuf.h"
#include "mmt_internal.h"
#include "mmt_sim3.h"

namespace mmt {

// a row of a cv::Mat product: the dot product summed in double, rounded to float
__device__ __forceinline__ float dot3d(float a0, float a1, float a2, float b0, float b1,
                                       float b2) {
  double s = (double)a0 * (double)b0;
  s += (double)a1 * (double)b1;
  s += (double)a2 * (double)b2;
  return (float)s;
}

// one rotation of the cyclic Jacobi method on the symmetric 4 x 4 A (eigenvectors accumulated in
// the columns of V); P, Q compile-time so that A and V stay in registers
template <int P, int Q>
__device__ __forceinline__ void jacobi_rot(double (&A)[4][4], double (&V)[4][4]) {
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
  const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const double akp = A[k][P], akq = A[k][Q];
    A[k][P] = c * akp - s * akq;
    A[k][Q] = s * akp + c * akq;
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const double apk = A[P][k], aqk = A[Q][k];
    A[P][k] = c * apk - s * aqk;
    A[Q][k] = s * apk + c * aqk;
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const double vkp = V[k][P], vkq = V[k][Q];
    V[k][P] = c * vkp - s * vkq;
    V[k][Q] = s * vkp + c * vkq;
  }
}

// cv::eigen(N)'s first eigenvector as pinned: double Jacobi on the float entries, swept until the
// off-diagonal norm is below 1e-15 |N| (30 sweeps at most); the eigenvector of the largest
// eigenvalue, unit norm, its first non-zero component positive, rounded to float
__device__ __forceinline__ void top_quaternion(const float (&Nf)[4][4], float (&q)[4]) {
  double A[4][4], V[4][4];
  double nrm2 = 0;
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 4; c++) {
      A[r][c] = (double)Nf[r][c];
      V[r][c] = r == c ? 1.0 : 0.0;
      nrm2 += A[r][c] * A[r][c];
    }
  const double tol2 = 1e-30 * nrm2;
  for (int sweep = 0; sweep < 30; sweep++) {
    double off2 = 0;
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int c = 0; c < 4; c++)
        if (r != c) off2 += A[r][c] * A[r][c];
    if (off2 <= tol2) break;
    jacobi_rot<0, 1>(A, V);
    jacobi_rot<0, 2>(A, V);
    jacobi_rot<0, 3>(A, V);
    jacobi_rot<1, 2>(A, V);
    jacobi_rot<1, 3>(A, V);
    jacobi_rot<2, 3>(A, V);
  }
  double best = A[0][0];
  double e[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
  for (int j = 1; j < 4; j++)
    if (A[j][j] > best) {
      best = A[j][j];
#pragma unroll
      for (int k = 0; k < 4; k++) e[k] = V[k][j];
    }
  const double in = 1.0 / sqrt(((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) + e[3] * e[3]);
  double sgn = 1.0;
  if (e[0] != 0) sgn = e[0] < 0 ? -1.0 : 1.0;
  else if (e[1] != 0) sgn = e[1] < 0 ? -1.0 : 1.0;
  else if (e[2] != 0) sgn = e[2] < 0 ? -1.0 : 1.0;
  else if (e[3] != 0) sgn = e[3] < 0 ? -1.0 : 1.0;
#pragma unroll
  for (int k = 0; k < 4; k++) q[k] = (float)(sgn * (e[k] * in));
}

__global__ __launch_bounds__(64) void k_sim3_hyp(Sim3Args a) {
  const int h = blockIdx.x * 64 + threadIdx.x;
  if (h >= a.n_hyp) return;
  const Sim3SolverDev S = a.sol[a.hsol[h]];
  // the minimal set: columns of P3Dc1i / P3Dc2i
  float P1[3][3], P2[3][3];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const size_t row = 3 * (size_t)(S.pt_off + a.sub[3 * (size_t)h + j]);
#pragma unroll
    for (int r = 0; r < 3; r++) {
      P1[r][j] = a.X1[row + r];
      P2[r][j] = a.X2[row + r];
    }
  }
  // ComputeCentroid: float row sums divided by the column count
  float O1[3], O2[3], Pr1[3][3], Pr2[3][3];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    O1[r] = ((P1[r][0] + P1[r][1]) + P1[r][2]) / 3.0f;
    O2[r] = ((P2[r][0] + P2[r][1]) + P2[r][2]) / 3.0f;
#pragma unroll
    for (int j = 0; j < 3; j++) {
      Pr1[r][j] = P1[r][j] - O1[r];
      Pr2[r][j] = P2[r][j] - O2[r];
    }
  }
  float M[3][3];  // Pr2 * Pr1^T
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++)
      M[i][j] = dot3d(Pr2[i][0], Pr2[i][1], Pr2[i][2], Pr1[j][0], Pr1[j][1], Pr1[j][2]);
  const float N11 = (M[0][0] + M[1][1]) + M[2][2];
  const float N12 = M[1][2] - M[2][1];
  const float N13 = M[2][0] - M[0][2];
  const float N14 = M[0][1] - M[1][0];
  const float N22 = (M[0][0] - M[1][1]) - M[2][2];
  const float N23 = M[0][1] + M[1][0];
  const float N24 = M[2][0] + M[0][2];
  const float N33 = (-M[0][0] + M[1][1]) - M[2][2];
  const float N34 = M[1][2] + M[2][1];
  const float N44 = (-M[0][0] - M[1][1]) + M[2][2];
  const float Nf[4][4] = {{N11, N12, N13, N14}, {N12, N22, N23, N24}, {N13, N23, N33, N34},
                          {N14, N24, N34, N44}};
  float q[4];
  top_quaternion(Nf, q);
  // angle-axis: sin is the norm of the imaginary part, cos the real part; the quaternion angle is
  // half the rotation's.  A zero imaginary part divides 0 by 0 as the reference does.
  const double vn = sqrt(((double)q[1] * (double)q[1] + (double)q[2] * (double)q[2]) +
                         (double)q[3] * (double)q[3]);
  const double ang = atan2(vn, (double)q[0]);
  double rv[3];
#pragma unroll
  for (int k = 0; k < 3; k++) rv[k] = ((2.0 * ang) * (double)q[1 + k]) / vn;
  // cv::Rodrigues: cos I + (1 - cos) k k^T + sin [k]x
  const double theta = sqrt((rv[0] * rv[0] + rv[1] * rv[1]) + rv[2] * rv[2]);
  const double kx[3] = {rv[0] / theta, rv[1] / theta, rv[2] / theta};
  const double ct = cos(theta), sn = sin(theta);
  const double Kx[3][3] = {{0.0, -kx[2], kx[1]}, {kx[2], 0.0, -kx[0]}, {-kx[1], kx[0], 0.0}};
  float R[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++)
      R[i][j] = (float)(((i == j ? ct : 0.0) + ((1.0 - ct) * kx[i]) * kx[j]) + sn * Kx[i][j]);
  // scale: nom = Pr1 . (R Pr2), den = the squares of R Pr2, both summed in double
  float s = 1.0f;
  if (!S.fix_scale) {
    double nom = 0, den = 0;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const float p3 = dot3d(R[i][0], R[i][1], R[i][2], Pr2[0][k], Pr2[1][k], Pr2[2][k]);
        nom += (double)Pr1[i][k] * (double)p3;
        den += (double)(p3 * p3);
      }
    s = (float)(nom / den);
  }
  Sim3Hyp H;
  const double inv = 1.0 / (double)s;
  float sR[3][3], sRi[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      sR[i][j] = s * R[i][j];
      sRi[i][j] = (float)(inv * (double)R[j][i]);
      H.R[3 * i + j] = R[i][j];
    }
#pragma unroll
  for (int i = 0; i < 3; i++) {  // t12 = O1 - s R O2
    H.t[i] = O1[i] - dot3d(sR[i][0], sR[i][1], sR[i][2], O2[0], O2[1], O2[2]);
#pragma unroll
    for (int j = 0; j < 3; j++) H.T12[4 * i + j] = sR[i][j];
    H.T12[4 * i + 3] = H.t[i];
  }
#pragma unroll
  for (int i = 0; i < 3; i++) {  // t21 = -(1/s R^T) t12
#pragma unroll
    for (int j = 0; j < 3; j++) H.T21[4 * i + j] = sRi[i][j];
    H.T21[4 * i + 3] = -dot3d(sRi[i][0], sRi[i][1], sRi[i][2], H.t[0], H.t[1], H.t[2]);
  }
  H.s = s;
  H.pad[0] = H.pad[1] = H.pad[2] = 0;
  a.hyp[h] = H;
}

// Sim3Solver::Project of one point with the 3 x 4 rows T: (u, v)
__device__ __forceinline__ void sim3_project(const float* T, float x, float y, float z, float fx,
                                             float fy, float cx, float cy, float& u, float& v) {
  const float px = dot3d(T[0], T[1], T[2], x, y, z) + T[3];
  const float py = dot3d(T[4], T[5], T[6], x, y, z) + T[7];
  const float pz = dot3d(T[8], T[9], T[10], x, y, z) + T[11];
  const float invz = 1 / pz;
  u = fx * (px * invz) + cx;
  v = fy * (py * invz) + cy;
}

__global__ __launch_bounds__(kSim3ScoreThreads) void k_sim3_score(Sim3Args a) {
  __shared__ int s_w[kSim3ScoreThreads / 64];
  const int h = blockIdx.x;
  const Sim3SolverDev& S = a.sol[a.hsol[h]];
  const Sim3Hyp& H = a.hyp[h];
  const int n = S.n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint8_t* fl = a.flags + S.flag_off + (size_t)(h - S.hyp_off) * (size_t)n;
  int cnt = 0;
  for (int i0 = 0; i0 < n; i0 += kSim3ScoreThreads) {  // uniform bound: every wave votes
    const int i = i0 + threadIdx.x;
    bool in = false;
    if (i < n) {
      const size_t p = (size_t)(S.pt_off + i);
      const float x1 = a.X1[3 * p], y1 = a.X1[3 * p + 1], z1 = a.X1[3 * p + 2];
      const float x2 = a.X2[3 * p], y2 = a.X2[3 * p + 1], z2 = a.X2[3 * p + 2];
      // mvP1im1 / mvP2im2 (FromCameraToImage)
      const float iz1 = 1 / z1, iz2 = 1 / z2;
      const float u11 = S.fx1 * (x1 * iz1) + S.cx1, v11 = S.fy1 * (y1 * iz1) + S.cy1;
      const float u22 = S.fx2 * (x2 * iz2) + S.cx2, v22 = S.fy2 * (y2 * iz2) + S.cy2;
      float u21, v21, u12, v12;
      sim3_project(H.T12, x2, y2, z2, S.fx1, S.fy1, S.cx1, S.cy1, u21, v21);  // vP2im1
      sim3_project(H.T21, x1, y1, z1, S.fx2, S.fy2, S.cx2, S.cy2, u12, v12);  // vP1im2
      const float dx1 = u11 - u21, dy1 = v11 - v21;
      const float dx2 = u12 - u22, dy2 = v12 - v22;
      const float err1 = (float)((double)dx1 * (double)dx1 + (double)dy1 * (double)dy1);
      const float err2 = (float)((double)dx2 * (double)dx2 + (double)dy2 * (double)dy2);
      in = err1 < a.max_err1[p] && err2 < a.max_err2[p];
      fl[i] = in ? 1 : 0;
    }
    cnt += __popcll(__ballot(in));
  }
  if (lane == 0) s_w[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
    for (int w = 0; w < kSim3ScoreThreads / 64; w++) tot += s_w[w];
    a.count[h] = tot;
  }
}

void launch_sim3(const Sim3Args& a, hipStream_t st) {
  if (a.n_hyp <= 0) return;
  hipLaunchKernelGGL(k_sim3_hyp, dim3((a.n_hyp + 63) / 64), dim3(64), 0, st, a);
  MMT_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_sim3_score, dim3(a.n_hyp), dim3(kSim3ScoreThreads), 0, st, a);
  MMT_HIP(hipGetLastError());
}

namespace {

// double -> int as x86 converts it: NaN and out-of-range values give INT_MIN
int cvt_int(double v) {
  if (!(v > -2147483649.0 && v < 2147483648.0)) return INT_MIN;
  return (int)v;
}

// mRansacMaxIts of SetRansacParameters (Sim3Solver.cc:114-138)
int sim3_max_iterations(const mmt_sim3_problem& pr) {
  const float epsilon = (float)pr.min_inliers / (float)pr.n;
  int nIterations;
  if (pr.min_inliers == pr.n)
    nIterations = 1;
  else
    nIterations = cvt_int(std::ceil(std::log(1 - pr.probability) /
                                    std::log(1 - std::pow((double)epsilon, 3.0))));
  return std::max(1, std::min(nIterations, pr.max_iterations));
}

// mvnMaxError: 9.210 * sigmaSquare stored in a vector<size_t>, read back as a float by the
// comparison with the float error
float sim3_max_error(float sigma2) {
  if (!(sigma2 >= 0.f) || !(sigma2 < 1e15f)) throw ArgError("Sim3Solver: sigma2 out of range");
  return (float)(size_t)(9.210 * (double)sigma2);
}

void hyp_to_T(const Sim3Hyp& H, float* T) {
  memcpy(T, H.T12, 48);
  T[12] = T[13] = T[14] = 0.f;
  T[15] = 1.f;
}

}  // namespace

void sim3solver_iterate_gpu(hipStream_t s, int n_solvers, const mmt_sim3_problem* problems,
                            const int32_t* const* randi, const int32_t* n_draw_iters,
                            int n_iterations, mmt_sim3_state* states, mmt_sim3_result* results,
                            mmt_sim3_probe* probes) {
  if (n_solvers < 0 || n_solvers > kSim3MaxSolvers)
    throw ArgError("Sim3Solver: more than 64 solvers in one call");
  if (n_iterations < 0 || n_iterations > kSim3MaxIters)
    throw ArgError("Sim3Solver: more than 300 iterations in one call");
  std::vector<Sim3SolverDev> sol(std::max(n_solvers, 1));
  std::vector<int> maxIts(std::max(n_solvers, 1)), K(std::max(n_solvers, 1), 0);
  std::vector<int> hsol, sub, avail;
  size_t n_pts = 0, n_flags = 0;
  for (int i = 0; i < n_solvers; i++) {
    const mmt_sim3_problem& pr = problems[i];
    mmt_sim3_result& r = results[i];
    if (pr.n < 0 || pr.n > 16384) throw ArgError("Sim3Solver: n outside [0, 16384]");
    if (pr.n > 0 && (!pr.X1 || !pr.X2 || !pr.sigma2_1 || !pr.sigma2_2 || !states[i].best_mask ||
                     !r.inliers))
      throw ArgError("Sim3Solver: null problem, state or result arrays");
    r.found = r.n_inliers = r.no_more = 0;
    memset(r.T12, 0, sizeof(r.T12));
    if (pr.n > 0) memset(r.inliers, 0, (size_t)pr.n);
    if (probes) probes[i].n_hyp = 0;
    Sim3SolverDev& S = sol[i];
    memset(&S, 0, sizeof(S));
    S.n = pr.n;
    S.pt_off = (int)n_pts;
    S.hyp_off = (int)hsol.size();
    S.fix_scale = pr.fix_scale ? 1 : 0;
    S.flag_off = (long long)n_flags;
    S.fx1 = pr.fx1; S.fy1 = pr.fy1; S.cx1 = pr.cx1; S.cy1 = pr.cy1;
    S.fx2 = pr.fx2; S.fy2 = pr.fy2; S.cx2 = pr.cx2; S.cy2 = pr.cy2;
    n_pts += (size_t)pr.n;
    maxIts[i] = sim3_max_iterations(pr);
    if (pr.n < pr.min_inliers) {  // iterate(): bNoMore, nothing run, no draw consumed
      r.no_more = 1;
      continue;
    }
    if (pr.n < 3) throw ArgError("Sim3Solver: fewer than 3 correspondences to draw from");
    // while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations)
    K[i] = std::max(0, std::min(n_iterations, maxIts[i] - states[i].iterations));
    if (K[i] > 0 && (!randi || !n_draw_iters || !randi[i] || K[i] > n_draw_iters[i]))
      throw ArgError("Sim3Solver: randi covers fewer iterations than the call runs");
    // minimal sets: RandomInt draws through vAvailableIndices' swap-with-back removal
    avail.resize(pr.n);
    for (int k = 0; k < K[i]; k++) {
      for (int j = 0; j < pr.n; j++) avail[j] = j;
      int sz = pr.n;
      for (int j = 0; j < 3; j++) {
        const int d = randi[i][3 * (size_t)k + j];
        if (d < 0 || d >= sz) throw ArgError("Sim3Solver: randi value outside [0, n-1-j]");
        sub.push_back(avail[d]);
        avail[d] = avail[sz - 1];
        sz--;
      }
      hsol.push_back(i);
    }
    n_flags += (size_t)K[i] * (size_t)pr.n;
  }
  const int n_hyp = (int)hsol.size();
  std::vector<int> h_count(std::max(n_hyp, 1));
  std::vector<Sim3Hyp> h_hyp(std::max(n_hyp, 1));
  DevBuf<uint8_t> d_flags(n_flags);
  if (n_hyp > 0) {
    std::vector<float> X1(3 * n_pts), X2(3 * n_pts), e1(n_pts), e2(n_pts);
    for (int i = 0; i < n_solvers; i++) {
      const mmt_sim3_problem& pr = problems[i];
      if (pr.n == 0) continue;
      const size_t o = (size_t)sol[i].pt_off;
      memcpy(&X1[3 * o], pr.X1, 12 * (size_t)pr.n);
      memcpy(&X2[3 * o], pr.X2, 12 * (size_t)pr.n);
      for (int j = 0; j < pr.n; j++) {
        e1[o + j] = sim3_max_error(pr.sigma2_1[j]);
        e2[o + j] = sim3_max_error(pr.sigma2_2[j]);
      }
    }
    DevBuf<float> dX1(3 * n_pts), dX2(3 * n_pts), de1(n_pts), de2(n_pts);
    DevBuf<Sim3SolverDev> dsol(n_solvers);
    DevBuf<int> dhsol(n_hyp), dsub(3 * (size_t)n_hyp), dcount(n_hyp);
    DevBuf<Sim3Hyp> dhyp(n_hyp);
    dX1.up(X1, s);
    dX2.up(X2, s);
    de1.up(e1, s);
    de2.up(e2, s);
    dsol.up(sol.data(), n_solvers, s);
    dhsol.up(hsol, s);
    dsub.up(sub, s);
    Sim3Args a;
    a.sol = dsol.p;
    a.hsol = dhsol.p;
    a.sub = dsub.p;
    a.n_hyp = n_hyp;
    a.X1 = dX1.p;
    a.X2 = dX2.p;
    a.max_err1 = de1.p;
    a.max_err2 = de2.p;
    a.hyp = dhyp.p;
    a.flags = d_flags.p;
    a.count = dcount.p;
    launch_sim3(a, s);
    dcount.down(h_count.data(), n_hyp, s);
    dhyp.down(h_hyp.data(), n_hyp, s);
    MMT_HIP(hipStreamSynchronize(s));
  }
  // iterate()'s loop (Sim3Solver.cc:158-206) over the counts, hypothesis by hypothesis.  The best
  // set is copied on >=, so only the last copy of the call is fetched.
  for (int i = 0; i < n_solvers; i++) {
    const mmt_sim3_problem& pr = problems[i];
    mmt_sim3_state& st = states[i];
    mmt_sim3_result& r = results[i];
    if (pr.n < pr.min_inliers) continue;
    const int h0 = sol[i].hyp_off;
    int last = -1;
    for (int k = 0; k < K[i] && !r.found; k++) {
      st.iterations++;
      const int c = h_count[h0 + k];
      if (c >= st.best_inliers) {
        last = k;
        st.best_inliers = c;
        if (c > pr.min_inliers) r.found = 1;
      }
    }
    if (last >= 0) {
      const Sim3Hyp& H = h_hyp[h0 + last];
      d_flags.down_now(st.best_mask, pr.n,
                       (size_t)sol[i].flag_off + (size_t)last * (size_t)pr.n);
      hyp_to_T(H, st.best_T12);
      memcpy(st.best_R, H.R, sizeof(H.R));
      memcpy(st.best_t, H.t, sizeof(H.t));
      st.best_scale = H.s;
    }
    if (r.found) {
      r.n_inliers = st.best_inliers;
      memcpy(r.inliers, st.best_mask, (size_t)pr.n);
      memcpy(r.T12, st.best_T12, sizeof(r.T12));
    } else if (st.iterations >= maxIts[i]) {
      r.no_more = 1;
    }
    if (probes) {  // every hypothesis the call launched, whether or not the loop reached it
      mmt_sim3_probe& pb = probes[i];
      const int m = std::min(K[i], pb.cap);
      pb.n_hyp = m;
      for (int k = 0; k < m; k++) {
        if (pb.counts) pb.counts[k] = h_count[h0 + k];
        if (pb.T12) hyp_to_T(h_hyp[h0 + k], pb.T12 + 16 * (size_t)k);
      }
      if (pb.flags) d_flags.down_now(pb.flags, (size_t)m * (size_t)pr.n, sol[i].flag_off);
    }
  }
}

}  // namespace mmt
