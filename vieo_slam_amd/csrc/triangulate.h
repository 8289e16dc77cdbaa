// GeometricCamera::TriangulateMatches / Triangulate on the device (reference common/camera_models/camera_base.h:199-285,
// :576-608), shared by the fisheye stereo stage (null_vector4) and LocalMapping::CreateNewMapPoints (tri_search.hip).
// Eigen::JacobiSVD's last right singular vector (camera_base.h:599-600) is obtained by one-sided Jacobi rotations on
// the columns of A (FP64), which is branch-light and register resident for a 4-column matrix.
#pragma once
#include "ba_device.h"

namespace vieo {

// right singular vector of the smallest singular value of A (M x 4), one-sided Jacobi; A is destroyed
template <int M>
__device__ __forceinline__ void null_vector4(double (&A)[M][4], double* x4) {
  double V[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) V[r][c] = r == c ? 1. : 0.;
  for (int sweep = 0; sweep < 40; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        double a = 0, b = 0, g = 0;
#pragma unroll
        for (int r = 0; r < M; ++r) a += A[r][p] * A[r][p], b += A[r][q] * A[r][q], g += A[r][p] * A[r][q];
        if (g == 0 || fabs(g) <= 1e-15 * sqrt(a * b)) continue;
        rotated = true;
        const double zeta = (b - a) / (2 * g);
        const double t = (zeta >= 0 ? 1. : -1.) / (fabs(zeta) + sqrt(1 + zeta * zeta));
        const double cs = 1 / sqrt(1 + t * t), sn = cs * t;
#pragma unroll
        for (int r = 0; r < M; ++r) {
          const double u = A[r][p], v = A[r][q];
          A[r][p] = cs * u - sn * v, A[r][q] = sn * u + cs * v;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double u = V[r][p], v = V[r][q];
          V[r][p] = cs * u - sn * v, V[r][q] = sn * u + cs * v;
        }
      }
    if (!rotated) break;
  }
  double nb = INFINITY;
  x4[0] = x4[1] = x4[2] = x4[3] = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    double n = 0;
#pragma unroll
    for (int r = 0; r < M; ++r) n += A[r][c] * A[r][c];
    if (n < nb) {
      nb = n;
#pragma unroll
      for (int r = 0; r < 4; ++r) x4[r] = V[r][c];
    }
  }
}

// One observation of TriangulateMatches.  cam and Tcw point to global memory: a camera's coefficient array is indexed
// at run time, which a per-lane copy would pay for with scratch.
struct TriObs {
  bool on;            // false: the slot is empty (the reference's vectors simply do not hold it)
  const CamD* cam;
  const double* Tcw;  // world -> this camera, row-major 3x4 = (Twr * Trc).inverse(), inverted in double
  double nx, ny;      // UnProject(key point) on the plane z = 1
  float u, v;         // the key point
  float sigma2;       // vlevelsigma2_[octave]
  float uright, bf;   // purbf: uright == -1 = no third residual
};

// TriangulateMatches over at most N observations with world poses.  get(i) hands out slot i; it is called with
// compile-time i in the unrolled loops and with run-time i in the check loop, so it must read from memory, not from
// per-lane arrays.  Empty slots become zero rows of the DLT system, which changes no bit: the Jacobi sums gain terms
// + 0 * 0 and a rotation leaves a zero row zero.
//   thresh_cosdisparity  the parallax gate is taken only when it is < 1; the per-pair cosine is rounded to float
//   just_check_p3d       x3d is an input: no gate's DLT, only the depth and reprojection checks
// returns false for the reference's empty vector.  The depths czs are checked (float, > 0) but not handed back:
// CreateNewMapPoints only asks whether the vector is empty.
template <int N, class Get>
__device__ __forceinline__ bool triangulate_matches_world(Get get, float thresh_cosdisparity, bool just_check_p3d,
                                                          double* x3d) {
  if (thresh_cosdisparity < 1.f) {
    double w[N][3], px[N], py[N];  // Twi.so3() * normedcP, normedcP
    bool on[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const TriObs o = get(i);
      on[i] = o.on, px[i] = o.nx, py[i] = o.ny;
      const double* T = o.Tcw;
#pragma unroll
      for (int r = 0; r < 3; ++r) w[i][r] = o.on ? (T[r] * o.nx + T[4 + r] * o.ny) + T[8 + r] * 1.0 : 0.0;
    }
    bool bret = true;  // every pair has cos > thresh  =>  no usable parallax
#pragma unroll
    for (int i = 0; i < N - 1; ++i) {
      if (!on[i]) continue;
      const double* T = get(i).Tcw;
      const double R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
      const double ni = sqrt((px[i] * px[i] + py[i] * py[i]) + 1.0);
#pragma unroll
      for (int j = i + 1; j < N; ++j) {
        if (!on[j]) continue;
        double v[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) v[r] = (R[r * 3] * w[j][0] + R[r * 3 + 1] * w[j][1]) + R[r * 3 + 2] * w[j][2];
        const double dot = (px[i] * v[0] + py[i] * v[1]) + 1.0 * v[2];
        const double nj = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
        const float cosr = (float)(dot / (ni * nj));
        if (cosr <= thresh_cosdisparity) bret = false;
      }
    }
    if (bret) return false;
  }
  double X[3] = {x3d[0], x3d[1], x3d[2]};
  if (!just_check_p3d) {
    double A[2 * N][4];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const TriObs o = get(i);
      const double* T = o.Tcw;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        A[2 * i][c] = o.on ? o.nx * T[8 + c] - T[c] : 0.0;
        A[2 * i + 1][c] = o.on ? o.ny * T[8 + c] - T[4 + c] : 0.0;
      }
    }
    double x4[4];
    null_vector4<2 * N>(A, x4);
    if (!x4[3]) return false;
    X[0] = x4[0] / x4[3], X[1] = x4[1] / x4[3], X[2] = x4[2] / x4[3];
  }
#pragma unroll 1
  for (int i = 0; i < N; ++i) {
    const TriObs o = get(i);
    if (!o.on) continue;
    const double* T = o.Tcw;
    const float cz = (float)(((T[8] * X[0] + T[9] * X[1]) + T[10] * X[2]) + T[11]);
    if (cz <= 0) return false;
    double Pc[3], uv[2];
    for (int r = 0; r < 3; ++r) Pc[r] = ((T[r * 4] * X[0] + T[r * 4 + 1] * X[1]) + T[r * 4 + 2] * X[2]) + T[r * 4 + 3];
    cam_project(*o.cam, Pc, uv, nullptr);  // uv comes back rounded to float
    const float e0 = (float)uv[0] - o.u, e1 = (float)uv[1] - o.v;
    float err2 = e0 * e0 + e1 * e1, thresh_chi2 = 5.991f;
    if (o.uright != -1.f) {  // the stereo key's third residual, all of it float
      const float u2_r = (float)uv[0] - o.bf / cz;
      const float e2 = u2_r - o.uright;
      err2 = err2 + e2 * e2, thresh_chi2 = 7.8f;
    }
    if (err2 > thresh_chi2 * o.sigma2) return false;
  }
  x3d[0] = X[0], x3d[1] = X[1], x3d[2] = X[2];
  return true;
}

}  // namespace vieo
