// multimot_track_amd/csrc/mmt_mat4.h -- the float cv::Mat helpers of the tracker's pose
// bookkeeping, shared by host and device so the device-side motion-model matrix equals the host's
// bit for bit (double accumulation, float result; contraction is off in both compilations).
// Plain C++ outside hipcc (the map graph and its host test include it without the device headers).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MMT_HD __host__ __device__
#else
#define MMT_HD
#endif

#include <cmath>
#include <cstdint>
#include <cstring>

namespace mmt {

// cv::gemm, CV_32F: C = A B (4x4)
MMT_HD inline void mat4_mul(const float* A, const float* B, float* C) {
  float R[16];
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) {
      double s = 0;
      for (int k = 0; k < 4; k++) s += (double)A[4 * r + k] * (double)B[4 * k + c];
      R[4 * r + c] = (float)s;
    }
  for (int i = 0; i < 16; i++) C[i] = R[i];
}

// Tracking::InvMatrix: [R^T, -R^T t]
MMT_HD inline void inv_mat(const float* T, float* Ti) {
  float R[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) R[4 * r + c] = T[4 * c + r];
  for (int r = 0; r < 3; r++) {
    double s = 0;
    for (int k = 0; k < 3; k++) s += (double)T[4 * k + r] * (double)T[4 * k + 3];
    R[4 * r + 3] = (float)(-s);
  }
  for (int i = 0; i < 16; i++) Ti[i] = R[i];
}

MMT_HD inline void mat4_eye(float* T) {
  for (int i = 0; i < 16; i++) T[i] = (i % 5 == 0) ? 1.f : 0.f;
}

// ---- host only: the pose and descriptor helpers of the map code and the C-ABI probes (the
// matcher kernels keep their own pose_xform / pose_centre, mmt_match.hip)

// Frame::UpdatePoseMatrices / KeyFrame::SetPose: Ow = -Rcw^T tcw
inline void cam_centre(const float* T, float* Ow) {
  for (int r = 0; r < 3; r++) {
    double s = 0;
    for (int k = 0; k < 3; k++) s += (double)T[4 * k + r] * (double)T[4 * k + 3];
    Ow[r] = -(float)s;
  }
}

// y = R x + t of the pose T
inline void xform(const float* T, const float* x, float* y) {
  for (int r = 0; r < 3; r++) {
    double s = 0;
    for (int k = 0; k < 3; k++) s += (double)T[4 * r + k] * (double)x[k];
    y[r] = (float)s + T[4 * r + 3];
  }
}

// cv::norm of a 3-vector
inline float norm3(const float* v) {
  double s = 0;
  for (int k = 0; k < 3; k++) s += (double)v[k] * (double)v[k];
  return (float)std::sqrt(s);
}

// Frame / KeyFrame::UnprojectStereo (Frame.cc:1064-1079): Rwc * ((u - cx) z / fx,
// (v - cy) z / fy, z) + Ow; c is the camera record (MapCamH: cx, cy, invfx, invfy)
template <class Cam>
inline void unproject(const Cam& c, const float* T, float u, float v, float z, float* out) {
  const float x = (u - c.cx) * z * c.invfx;
  const float y = (v - c.cy) * z * c.invfy;
  const float xc[3] = {x, y, z};
  float Ow[3];
  cam_centre(T, Ow);
  for (int r = 0; r < 3; r++) {
    double s = 0;
    for (int k = 0; k < 3; k++) s += (double)T[4 * k + r] * (double)xc[k];
    out[r] = (float)s + Ow[r];
  }
}

// ORBmatcher::DescriptorDistance of two 32-byte descriptors
inline int hamming(const uint8_t* a, const uint8_t* b) {
  int d = 0;
  for (int i = 0; i < 4; i++) {
    uint64_t x, y;
    memcpy(&x, a + 8 * i, 8);
    memcpy(&y, b + 8 * i, 8);
    d += __builtin_popcountll(x ^ y);
  }
  return d;
}

}  // namespace mmt
