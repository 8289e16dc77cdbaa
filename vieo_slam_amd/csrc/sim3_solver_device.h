// sim3_solver_device.h -- the arithmetic of one Sim3Solver hypothesis (reference src/Sim3Solver.cc:220-373: ComputeSim3,
// CheckInliers, Project), written once for k_sim3_hypotheses of sim3_solver.hip.  FP64 from the float inputs.  Every
// array is indexed at compile time (the loops over rows, columns and Jacobi pairs unroll), so a hypothesis lives in
// registers.  The file also compiles as plain C++ (every lane function is then an ordinary inline function), which is
// how its arithmetic can be exercised on a host.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "cam_project.h"

#ifdef __HIPCC__
#define S3S_DEV __device__ __forceinline__
#else
#define S3S_DEV static inline
#endif

namespace vieo {

static const int kSim3MaxRows = 512;
static const int kSim3MaxCams = 8;

struct Sim3CandDev {
  int off, n;            // the candidate's correspondences in the concatenated arrays
  int words, mask_off;   // 64-bit words of one inlier mask (0: no solver); the candidate's first word in the mask table
  int cam_off1, cam_off2;  // pcams_[0] / pcams_[1] in the concatenated camera table
  int fix_scale, pad;
};

struct Sim3Pose {  // a hypothesis as CheckInliers reads it: mT12i = [s R | t], mT21i = [R^T / s | -R^T t / s]
  double A12[3][3], t12[3], A21[3][3], t21[3];
};

// the eigenvector of the largest eigenvalue of the symmetric 4 x 4 N (upper part read): cyclic Jacobi, the pairs in
// the fixed order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), so the result is the same run to run.  Neither its norm nor its
// sign matters to the caller.
S3S_DEV void s3s_top_eigenvector(const double (&N)[4][4], double (&q)[4]) {
  double A[4][4], V[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) A[i][j] = i <= j ? N[i][j] : N[j][i], V[i][j] = i == j ? 1. : 0.;
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int r = p + 1; r < 4; ++r) {
        const double g = A[p][r];
        if (g == 0) continue;
        const double h = 100 * fabs(g);
        if (fabs(A[p][p]) + h == fabs(A[p][p]) && fabs(A[r][r]) + h == fabs(A[r][r])) {
          A[p][r] = A[r][p] = 0;
          continue;
        }
        rotated = true;
        const double zeta = (A[r][r] - A[p][p]) / (2 * g);
        const double t = (zeta >= 0 ? 1. : -1.) / (fabs(zeta) + sqrt(1 + zeta * zeta));
        const double cs = 1 / sqrt(1 + t * t), sn = cs * t;
        A[p][p] -= t * g, A[r][r] += t * g, A[p][r] = A[r][p] = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (k != p && k != r) {
            const double u = A[k][p], v = A[k][r];
            A[k][p] = A[p][k] = cs * u - sn * v, A[k][r] = A[r][k] = sn * u + cs * v;
          }
          const double vp = V[k][p], vr = V[k][r];
          V[k][p] = cs * vp - sn * vr, V[k][r] = sn * vp + cs * vr;
        }
      }
    if (!rotated) break;
  }
  double best = A[0][0];
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = V[k][0];
#pragma unroll
  for (int c = 1; c < 4; ++c)
    if (A[c][c] > best) {
      best = A[c][c];
#pragma unroll
      for (int k = 0; k < 4; ++k) q[k] = V[k][c];
    }
}

// ComputeSim3 (:220-322) on 3 pairs: P1[i] / P2[i] = column i of P3Dc1i / P3Dc2i.  R, t, s = mR12i, mt12i, ms12i.
S3S_DEV void s3s_horn(const double (&P1)[3][3], const double (&P2)[3][3], bool fix_scale, double (&R)[3][3],
                      double (&t)[3], double& s) {
  // Step 1: centroids and relative coordinates
  double O1[3], O2[3], Pr1[3][3], Pr2[3][3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    O1[c] = ((P1[0][c] + P1[1][c]) + P1[2][c]) / 3, O2[c] = ((P2[0][c] + P2[1][c]) + P2[2][c]) / 3;
#pragma unroll
    for (int i = 0; i < 3; ++i) Pr1[i][c] = P1[i][c] - O1[c], Pr2[i][c] = P2[i][c] - O2[c];
  }
  // Step 2: M = Pr2 * Pr1^T
  double M[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) M[a][b] = (Pr2[0][a] * Pr1[0][b] + Pr2[1][a] * Pr1[1][b]) + Pr2[2][a] * Pr1[2][b];
  // Step 3: N
  double N[4][4];
  N[0][0] = (M[0][0] + M[1][1]) + M[2][2], N[0][1] = M[1][2] - M[2][1], N[0][2] = M[2][0] - M[0][2], N[0][3] = M[0][1] - M[1][0];
  N[1][1] = (M[0][0] - M[1][1]) - M[2][2], N[1][2] = M[0][1] + M[1][0], N[1][3] = M[2][0] + M[0][2];
  N[2][2] = (-M[0][0] + M[1][1]) - M[2][2], N[2][3] = M[1][2] + M[2][1];
  N[3][3] = (-M[0][0] - M[1][1]) + M[2][2];
  N[1][0] = N[2][0] = N[2][1] = N[3][0] = N[3][1] = N[3][2] = 0;  // (not read)
  // Step 4: the quaternion of the rotation, taken through the angle-axis form and cv::Rodrigues as the reference does;
  // an imaginary part of exactly zero (0 / 0 in the reference) is the identity
  double q[4];
  s3s_top_eigenvector(N, q);
  const double nv = sqrt((q[1] * q[1] + q[2] * q[2]) + q[3] * q[3]);
  const double ang = atan2(nv, q[0]);
  const double k = nv > 0 ? 2 * ang / nv : 0.0;
  const double rx = k * q[1], ry = k * q[2], rz = k * q[3];
  const double theta = sqrt((rx * rx + ry * ry) + rz * rz);
  if (theta < 2.220446049250313e-16) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) R[i][j] = i == j ? 1. : 0.;
  } else {
    const double c = cos(theta), sn = sin(theta), c1 = 1. - c, it = 1. / theta;
    const double x = rx * it, y = ry * it, z = rz * it;
    R[0][0] = c + c1 * x * x, R[0][1] = c1 * x * y - sn * z, R[0][2] = c1 * x * z + sn * y;
    R[1][0] = c1 * x * y + sn * z, R[1][1] = c + c1 * y * y, R[1][2] = c1 * y * z - sn * x;
    R[2][0] = c1 * x * z - sn * y, R[2][1] = c1 * y * z + sn * x, R[2][2] = c + c1 * z * z;
  }
  // Steps 5-6: rotate set 2, the scale
  if (!fix_scale) {
    double nom = 0, den = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double p3 = (R[r][0] * Pr2[i][0] + R[r][1] * Pr2[i][1]) + R[r][2] * Pr2[i][2];
        nom += Pr1[i][r] * p3, den += p3 * p3;
      }
    s = nom / den;
  } else
    s = 1.0;
  // Step 7: the translation
#pragma unroll
  for (int r = 0; r < 3; ++r) t[r] = O1[r] - s * ((R[r][0] * O2[0] + R[r][1] * O2[1]) + R[r][2] * O2[2]);
}

// Step 8: mT12i and mT21i
S3S_DEV void s3s_pose(const double (&R)[3][3], const double (&t)[3], double s, Sim3Pose& T) {
  const double is = 1.0 / s;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) T.A12[r][c] = s * R[r][c], T.A21[r][c] = is * R[c][r];
    T.t12[r] = t[r];
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) T.t21[r] = -((T.A21[r][0] * t[0] + T.A21[r][1] * t[1]) + T.A21[r][2] * t[2]);
}

// Project (:352-373) of one point: crP3D -- X itself, or A X + t rounded to float --, the camera's Tcr, its model; the
// image point is the float the reference returns
S3S_DEV void s3s_project(const CamD& cam, const double (*A)[3], const double* t, const float* __restrict__ X, float* uv) {
  double P[3] = {(double)X[0], (double)X[1], (double)X[2]};
  if (A) {
    const double x = P[0], y = P[1], z = P[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) P[r] = (double)(float)(((A[r][0] * x + A[r][1] * y) + A[r][2] * z) + t[r]);
  }
  double Pc[3], out[2];
#pragma unroll
  for (int r = 0; r < 3; ++r)
    Pc[r] = ((cam.Rcb[3 * r] * P[0] + cam.Rcb[3 * r + 1] * P[1]) + cam.Rcb[3 * r + 2] * P[2]) + cam.tcb[r];
  cam_project(cam, Pc, out, nullptr);
  uv[0] = (float)out[0], uv[1] = (float)out[1];
}

// the squared distance of two image points as cv::Mat::dot gives it to a float: float differences, their squares
// summed in double
S3S_DEV float s3s_dist2(const float* a, const float* b) {
  const float dx = a[0] - b[0], dy = a[1] - b[1];
  return (float)((double)dx * (double)dx + (double)dy * (double)dy);
}

// CheckInliers (:324-344) of one correspondence: X1 / X2 its two points, me1 / me2 the integer thresholds as floats
S3S_DEV bool s3s_is_inlier(const Sim3Pose& T, const CamD& cam1, const CamD& cam2, const float* __restrict__ X1,
                           const float* __restrict__ X2, float me1, float me2) {
  float p1im1[2], p2im2[2], p2im1[2], p1im2[2];
  s3s_project(cam1, nullptr, nullptr, X1, p1im1);
  s3s_project(cam2, nullptr, nullptr, X2, p2im2);
  s3s_project(cam1, T.A12, T.t12, X2, p2im1);
  s3s_project(cam2, T.A21, T.t21, X1, p1im2);
  const float err1 = s3s_dist2(p1im1, p2im1), err2 = s3s_dist2(p1im2, p2im2);
  return err1 < me1 && err2 < me2;
}

}  // namespace vieo
