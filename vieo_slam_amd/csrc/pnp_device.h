// pnp_device.h -- the arithmetic of one PnPsolver hypothesis (reference src/PnPsolver.cc:367-875: compute_pose and all
// it calls, CheckInliers), written once for the two kernels of pnp.hip.  sA / sV are the hypothesis' two 12 x 12
// work matrices, laid out [element][lane] (LDS on the device).  The file also compiles as plain C++ (every lane
// function is then an ordinary inline function), which is how its arithmetic can be exercised on a host.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#ifdef __HIPCC__
#define PNP_DEV __device__ __forceinline__
#else
#include <algorithm>
#define PNP_DEV static inline
#endif
#include "cam_project.h"

namespace vieo {

static const int kPnpLanes = 16;
static const int kPnpMaxRows = 512;

struct PnpCandDev {
  int off, n;  // the candidate's correspondences in the concatenated arrays
  float fx, fy, cx, cy;
  int words, mask_off;  // 64-bit words of one inlier mask; the candidate's first word in the pass-A mask table
};

// Frame::usedistort_: the cameras of the frame's rig.  One record per launch, read where it lies (global memory on the
// device): the camera of a correspondence is a run-time index, which costs a load there and scratch in registers.
struct PnpRigDev {
  int n_cams, reserved;
  CamD cams[4];                   // mpCameras[c], parameters widened once
  double Tcr[4][12], Trc[4][12];  // GetTcr() / GetTrc() as doubles, row-major 3 x 4
};

// what the rig instances of the two kernels read besides the rectified arrays (all null for the rectified ones):
// cam_of = mapidx2cami_ and usun, both concatenated like uv
struct PnpRigArgs {
  const PnpRigDev* rig;
  const unsigned char* cam_of;
  const double* usun;
};

struct PnpJob {  // pass B: one record
  int cand, idx_off, cnt, mask_off;
};

#define PNP_A(i, j) sA[((i) * 12 + (j)) * kPnpLanes + lane]
#define PNP_V(i, j) sV[((i) * 12 + (j)) * kPnpLanes + lane]
#define PNP_S(k) sA[(k) * kPnpLanes + lane]

// A test program may define PNP_TAP(slot, value) before including this file to record the values that decide
// pnp_epnp's branches (tests/hip_unit/solver_algebra_test.hip; slots listed there).  Undefined, as in the library, it
// expands to nothing and the code is the same text as without it.
#ifndef PNP_TAP
#define PNP_TAP(slot, value)
#endif

// least squares of a 6 x NC system by Householder reflections (cv::solve(DECOMP_SVD) / qr_solve of the reference: the
// same minimiser whenever the system has full column rank).  A and b are destroyed.  A column that is zero, or whose part
// outside the span of the columns before it is below 64 ulp of its own length, is moved behind the others, so that the
// remaining unknowns are still a minimiser over all six rows (an axis-aligned planar scene has two zero columns in the
// middle of the first initial guess), and of the minimisers the one of smallest norm is returned, the reference's.  At
// full rank no column moves and the arithmetic is that of the plain factorisation.
template <int NC>
PNP_DEV void pnp_lstsq6(double (&A)[6][NC], double (&b)[6], double (&x)[NC]) {
  constexpr double kTol2 = 0x1p-92;  // (64 * 2^-52)^2, against squared lengths
  double diag[NC], len2[NC], xp[NC];
  int col[NC];  // the column of the caller's A at each position
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    double s = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) s += A[i][j] * A[i][j];
    len2[j] = s, col[j] = j;
  }
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    double s = 0;
    for (int tries = 0;; ++tries) {
      s = 0;
#pragma unroll
      for (int i = k; i < 6; ++i) s += A[i][k] * A[i][k];
      if (s > kTol2 * len2[k] || tries >= NC - 1 - k) break;
      // nothing of this column is left: behind the others with it
      const double l = len2[k];
      const int c = col[k];
#pragma unroll
      for (int j = k; j < NC - 1; ++j) len2[j] = len2[j + 1], col[j] = col[j + 1];
      len2[NC - 1] = l, col[NC - 1] = c;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const double a = A[i][k];
#pragma unroll
        for (int j = k; j < NC - 1; ++j) A[i][j] = A[i][j + 1];
        A[i][NC - 1] = a;
      }
    }
    const double nrm = sqrt(s);
    diag[k] = 0;
    if (!(s > kTol2 * len2[k])) continue;
    const double alpha = A[k][k] > 0 ? -nrm : nrm;
    A[k][k] -= alpha;
    double vv = 0;
#pragma unroll
    for (int i = k; i < 6; ++i) vv += A[i][k] * A[i][k];
    diag[k] = alpha;
    if (!(vv > 0)) continue;
#pragma unroll
    for (int j = k + 1; j < NC; ++j) {
      double d = 0;
#pragma unroll
      for (int i = k; i < 6; ++i) d += A[i][k] * A[i][j];
      const double w = 2 * d / vv;
#pragma unroll
      for (int i = k; i < 6; ++i) A[i][j] -= w * A[i][k];
    }
    double d = 0;
#pragma unroll
    for (int i = k; i < 6; ++i) d += A[i][k] * b[i];
    const double w = 2 * d / vv;
#pragma unroll
    for (int i = k; i < 6; ++i) b[i] -= w * A[i][k];
  }
#pragma unroll
  for (int k = NC - 1; k >= 0; --k) {
    double s = b[k];
#pragma unroll
    for (int j = k + 1; j < NC; ++j) s -= A[k][j] * xp[j];
    xp[k] = diag[k] != 0 ? s / diag[k] : 0.0;
  }
  bool dropped = false;
#pragma unroll
  for (int k = 0; k < NC; ++k) dropped = dropped || diag[k] == 0;
  if (dropped) {
    // Without full rank the minimisers are a family xp - W y, y free in the dropped unknowns (W = R11^-1 R12).  The
    // reference's cv::solve(DECOMP_SVD) takes the one of smallest norm: (I + W^T W) y = W^T xp.
    double W[NC][NC], G[NC][NC], y[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j)
#pragma unroll
      for (int k = NC - 1; k >= 0; --k) {
        double s = k < j ? A[k][j] : 0.0;
#pragma unroll
        for (int l = k + 1; l < NC; ++l) s -= A[k][l] * W[l][j];
        W[k][j] = diag[j] == 0 && diag[k] != 0 && k < j ? s / diag[k] : 0.0;
      }
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      y[i] = 0;
#pragma unroll
      for (int k = 0; k < NC; ++k) y[i] += W[k][i] * xp[k];
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        G[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < NC; ++k) G[i][j] += W[k][i] * W[k][j];
      }
    }
#pragma unroll
    for (int p = 0; p < NC; ++p)  // symmetric, I + a Gram matrix: elimination without exchanges
#pragma unroll
      for (int i = p + 1; i < NC; ++i) {
        const double f = G[i][p] / G[p][p];
#pragma unroll
        for (int j = p; j < NC; ++j) G[i][j] -= f * G[p][j];
        y[i] -= f * y[p];
      }
#pragma unroll
    for (int p = NC - 1; p >= 0; --p) {
#pragma unroll
      for (int j = p + 1; j < NC; ++j) y[p] -= G[p][j] * y[j];
      y[p] /= G[p][p];
    }
#pragma unroll
    for (int k = 0; k < NC; ++k) {
#pragma unroll
      for (int j = 0; j < NC; ++j) xp[k] -= W[k][j] * y[j];
      if (diag[k] == 0) xp[k] = y[k];
    }
  }
#pragma unroll
  for (int j = 0; j < NC; ++j)
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (col[j] == c) x[c] = xp[j];
}

// one rotation angle of a Jacobi method: tan, cos, sin that annihilate the off-diagonal g between diagonals a and b
PNP_DEV void pnp_rot(double a, double b, double g, double& t, double& cs, double& sn) {
  const double zeta = (b - a) / (2 * g);
  t = (zeta >= 0 ? 1. : -1.) / (fabs(zeta) + sqrt(1 + zeta * zeta));
  cs = 1 / sqrt(1 + t * t), sn = cs * t;
}

// eigen-decomposition of the symmetric 3 x 3 S (upper part read): d descending, U[r][c] = component r of vector c
PNP_DEV void pnp_eig3(const double (&S)[3][3], double (&d)[3], double (&U)[3][3]) {
  double A[3][3] = {{S[0][0], S[0][1], S[0][2]}, {S[0][1], S[1][1], S[1][2]}, {S[0][2], S[1][2], S[2][2]}};
  double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = p + 1; q < 3; ++q) {
        const double g = A[p][q];
        if (g == 0) continue;
        const double h = 100 * fabs(g);
        if (fabs(A[p][p]) + h == fabs(A[p][p]) && fabs(A[q][q]) + h == fabs(A[q][q])) {
          A[p][q] = A[q][p] = 0;
          continue;
        }
        rotated = true;
        double t, cs, sn;
        pnp_rot(A[p][p], A[q][q], g, t, cs, sn);
        A[p][p] -= t * g, A[q][q] += t * g, A[p][q] = A[q][p] = 0;
        const int k = 3 - p - q;
        const double u = A[k][p], v = A[k][q];
        A[k][p] = A[p][k] = cs * u - sn * v, A[k][q] = A[q][k] = sn * u + cs * v;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const double vp = V[r][p], vq = V[r][q];
          V[r][p] = cs * vp - sn * vq, V[r][q] = sn * vp + cs * vq;
        }
      }
    if (!rotated) break;
  }
  // descending order by three compare-exchanges on (value, column)
  double e[3] = {A[0][0], A[1][1], A[2][2]};
#define PNP_CSWAP(i, j)                                                        \
  if (e[i] < e[j]) {                                                           \
    double w = e[i];                                                           \
    e[i] = e[j], e[j] = w;                                                     \
    for (int r = 0; r < 3; ++r) w = V[r][i], V[r][i] = V[r][j], V[r][j] = w;   \
  }
  PNP_CSWAP(0, 1)
  PNP_CSWAP(1, 2)
  PNP_CSWAP(0, 1)
#undef PNP_CSWAP
  // the sign of a principal direction is an internal matter of the reference's cv::SVD, and with noisy image points
  // the pose depends on it at the noise level: fixed here so that the component of largest magnitude is positive
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    d[c] = e[c];
    double big = V[0][c];
    if (fabs(V[1][c]) > fabs(big)) big = V[1][c];
    if (fabs(V[2][c]) > fabs(big)) big = V[2][c];
    const double sg = big < 0 ? -1. : 1.;
#pragma unroll
    for (int r = 0; r < 3; ++r) U[r][c] = sg * V[r][c];
  }
}

// R = U * V^T of the SVD of B (estimate_R_and_t): the orthogonal polar factor.  One-sided Jacobi on the columns of B
// gives B * V = U * Sigma; U is rebuilt from the two longest columns by Gram-Schmidt and the third as their cross
// product with the sign of the computed column, so R is orthogonal to round-off also when B is close to rank 2; where
// that column vanishes altogether, with the sign that makes R a rotation.
PNP_DEV void pnp_polar3(double (&B)[3][3], double (&R)[3][3]) {
  double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = p + 1; q < 3; ++q) {
        double a = 0, b = 0, g = 0;
#pragma unroll
        for (int r = 0; r < 3; ++r) a += B[r][p] * B[r][p], b += B[r][q] * B[r][q], g += B[r][p] * B[r][q];
        if (g == 0 || fabs(g) <= 1e-15 * sqrt(a * b)) continue;
        rotated = true;
        double t, cs, sn;
        pnp_rot(a, b, g, t, cs, sn);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const double u = B[r][p], v = B[r][q];
          B[r][p] = cs * u - sn * v, B[r][q] = sn * u + cs * v;
          const double vp = V[r][p], vq = V[r][q];
          V[r][p] = cs * vp - sn * vq, V[r][q] = sn * vp + cs * vq;
        }
      }
    if (!rotated) break;
  }
  double n2[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) n2[c] = (B[0][c] * B[0][c] + B[1][c] * B[1][c]) + B[2][c] * B[2][c];
  // longest column first (compare-exchanges on whole columns: no run-time register index)
#define PNP_CSWAP(i, j)                                          \
  if (n2[i] < n2[j]) {                                           \
    double w = n2[i];                                            \
    n2[i] = n2[j], n2[j] = w;                                    \
    for (int r = 0; r < 3; ++r) {                                \
      w = B[r][i], B[r][i] = B[r][j], B[r][j] = w;               \
      w = V[r][i], V[r][i] = V[r][j], V[r][j] = w;               \
    }                                                            \
  }
  PNP_CSWAP(0, 1)
  PNP_CSWAP(1, 2)
  PNP_CSWAP(0, 1)
#undef PNP_CSWAP
  double U[3][3];
  double c0[3], c1[3], c2[3], v0[3], v1[3], v2[3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
    c0[r] = B[r][0], c1[r] = B[r][1], c2[r] = B[r][2], v0[r] = V[r][0], v1[r] = V[r][1], v2[r] = V[r][2];
  const double l0 = sqrt((c0[0] * c0[0] + c0[1] * c0[1]) + c0[2] * c0[2]);
#pragma unroll
  for (int r = 0; r < 3; ++r) U[r][0] = c0[r] / l0;
  const double d01 = (c1[0] * U[0][0] + c1[1] * U[1][0]) + c1[2] * U[2][0];
#pragma unroll
  for (int r = 0; r < 3; ++r) c1[r] -= d01 * U[r][0];
  const double l1 = sqrt((c1[0] * c1[0] + c1[1] * c1[1]) + c1[2] * c1[2]);
#pragma unroll
  for (int r = 0; r < 3; ++r) U[r][1] = c1[r] / l1;
  double x[3] = {U[1][0] * U[2][1] - U[2][0] * U[1][1], U[2][0] * U[0][1] - U[0][0] * U[2][1],
                 U[0][0] * U[1][1] - U[1][0] * U[0][1]};
  const double along = (x[0] * c2[0] + x[1] * c2[1]) + x[2] * c2[2];
  double sg = along < 0 ? -1. : 1.;
  if (along == 0) {
    // B has rank 2 to the last bit (map points in a plane z = const: a zero column): the third direction is not B's
    // to give, and a reflection here would be "mended" by the caller's row flip into a wrong pose.  The rotation: det V
    const double dv = (v0[0] * (v1[1] * v2[2] - v1[2] * v2[1]) - v0[1] * (v1[0] * v2[2] - v1[2] * v2[0])) +
                      v0[2] * (v1[0] * v2[1] - v1[1] * v2[0]);
    sg = dv < 0 ? -1. : 1.;
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) U[r][2] = sg * x[r];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R[i][j] = (U[i][0] * v0[j] + U[i][1] * v1[j]) + U[i][2] * v2[j];
}

struct PnpFrame {  // what every pass over the correspondences needs to rebuild a point's barycentric coordinates
  double c0[3];     // cws[0]
  double ci[3][3];  // CC^-1
};

PNP_DEV void pnp_alphas(const PnpFrame& F, const float* __restrict__ X, double* a) {
  const double d0 = (double)X[0] - F.c0[0], d1 = (double)X[1] - F.c0[1], d2 = (double)X[2] - F.c0[2];
#pragma unroll
  for (int j = 0; j < 3; ++j) a[1 + j] = (F.ci[j][0] * d0 + F.ci[j][1] * d1) + F.ci[j][2] * d2;
  a[0] = ((1.0 - a[1]) - a[2]) - a[3];
}

// Getuv of the rectified configuration: invZc is a float
PNP_DEV void pnp_project(const PnpCandDev& C, const double (&R)[3][3], const double (&t)[3],
                                            const float* __restrict__ X, double& ue, double& ve) {
  double P[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) P[r] = ((R[r][0] * (double)X[0] + R[r][1] * (double)X[1]) + R[r][2] * (double)X[2]) + t[r];
  const float invz = (float)(1. / P[2]);
  ue = (double)C.cx + ((double)C.fx * P[0]) * (double)invz;
  ve = (double)C.cy + ((double)C.fy * P[1]) * (double)invz;
}

// a point of the reference camera in camera `cam` of the rig: Tcr * P
PNP_DEV void pnp_rig_transform(const double* __restrict__ T, const double* P, double* Q) {
#pragma unroll
  for (int r = 0; r < 3; ++r) Q[r] = ((T[4 * r] * P[0] + T[4 * r + 1] * P[1]) + T[4 * r + 2] * P[2]) + T[4 * r + 3];
}

// Getuv with Frame::usedistort_ (PnPsolver.cc:283-290): Pc = GetTcr() * Pcr of the correspondence's camera, then that
// camera model's Project, whose image point is a float.  A pixel that is not finite (z = 0 under Radtan, a quotient
// that overflows) stays so: the comparisons of both callers are then false.
PNP_DEV void pnp_project_rig(const PnpRigDev& G, int cam, const double (&R)[3][3], const double (&t)[3],
                             const float* __restrict__ X, double& ue, double& ve) {
  double P[3], Pc[3], px[2];
#pragma unroll
  for (int r = 0; r < 3; ++r) P[r] = ((R[r][0] * (double)X[0] + R[r][1] * (double)X[1]) + R[r][2] * (double)X[2]) + t[r];
  pnp_rig_transform(G.Tcr[cam], P, Pc);
  cam_project(G.cams[cam], Pc, px, nullptr);
  ue = px[0], ve = px[1];
}

// compute_pose over the cnt correspondences idx[0..cnt) of candidate C.  RIG: fill_M reads usun where the rectified form
// reads the pixel, reprojection_error compares the raw pixel with the rig Getuv.
template <bool RIG>
PNP_DEV void pnp_epnp_t(const PnpCandDev& C, const PnpRigArgs& G, const float* __restrict__ Xw, const float* __restrict__ uv,
                                      const int* __restrict__ idx, int cnt, double* sA, double* sV, int lane,
                                      double (&Rout)[3][3], double (&tout)[3]) {
  const float* Xc = Xw + 3 * (size_t)C.off;
  const float* Uc = uv + 2 * (size_t)C.off;
  const double* Un = nullptr;           // usun
  const unsigned char* Cam = nullptr;   // mapidx2cami_
  if constexpr (RIG) Un = G.usun + 2 * (size_t)C.off, Cam = G.cam_of + (size_t)C.off;
  // ---- choose_control_points, compute_barycentric_coordinates
  // The control points are kept as offsets from the centroid: the barycentric coordinates below are those of
  // centroid + offset exactly, and rho has to be the distances of the same points.  Adding the centroid first rounds
  // each point to the scale of the world's coordinates (1e-12 of a metre-sized offset at 1e4 m), which the pose then
  // shows a hundredfold.
  PnpFrame F;
  double co[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  {
    double s[3] = {0, 0, 0};
    for (int i = 0; i < cnt; ++i) {
      const float* X = Xc + 3 * idx[i];
      s[0] += (double)X[0], s[1] += (double)X[1], s[2] += (double)X[2];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) F.c0[r] = s[r] / cnt;
    double S[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int i = 0; i < cnt; ++i) {
      const float* X = Xc + 3 * idx[i];
      const double d[3] = {(double)X[0] - F.c0[0], (double)X[1] - F.c0[1], (double)X[2] - F.c0[2]};
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = r; c < 3; ++c) S[r][c] += d[r] * d[c];
    }
    double dc[3], U[3][3];
    pnp_eig3(S, dc, U);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double k = sqrt(fmax(dc[j], 0.0) / cnt);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        co[1 + j][r] = k * U[r][j];
        F.ci[j][r] = k > 0 ? U[r][j] / k : 0.0;  // CC = [k_j u_j]: its (pseudo-)inverse has the rows u_j / k_j
      }
    }
  }
  // ---- MtM: the two rows of a correspondence are a_i * (fu, 0, uc - u) and a_i * (0, fv, vc - v) per control point,
  // so a 3 x 3 block (i, j) of MtM is made of four sums over the correspondences
  {
    double s0[10], s1[10], s2[10], s3[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) s0[k] = s1[k] = s2[k] = s3[k] = 0;
    for (int i = 0; i < cnt; ++i) {
      const int g = idx[i];
      double a[4];
      pnp_alphas(F, Xc + 3 * g, a);
      double du, dv;
      if constexpr (RIG)
        du = (double)C.cx - Un[2 * g], dv = (double)C.cy - Un[2 * g + 1];
      else
        du = (double)C.cx - (double)Uc[2 * g], dv = (double)C.cy - (double)Uc[2 * g + 1];
      const double dd = du * du + dv * dv;
      int k = 0;
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = p; q < 4; ++q, ++k) {
          const double w = a[p] * a[q];
          s0[k] += w, s1[k] += w * du, s2[k] += w * dv, s3[k] += w * dd;
        }
    }
    const double fx = C.fx, fy = C.fy;
    int k = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int q = p; q < 4; ++q, ++k) {
        const double b[3][3] = {{fx * fx * s0[k], 0, fx * s1[k]}, {0, fy * fy * s0[k], fy * s2[k]}, {fx * s1[k], fy * s2[k], s3[k]}};
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c) PNP_A(3 * p + r, 3 * q + c) = b[r][c], PNP_A(3 * q + c, 3 * p + r) = b[r][c];
      }
#pragma unroll 1
    for (int r = 0; r < 12; ++r)
#pragma unroll 1
      for (int c = 0; c < 12; ++c) PNP_V(r, c) = r == c ? 1. : 0.;
  }
  // ---- eigenvectors of MtM: cyclic Jacobi, pairs (p, q) row by row; row e of sV becomes the vector of diagonal e
#pragma unroll 1
  for (int sweep = 0; sweep < 24; ++sweep) {
    bool rotated = false;
#pragma unroll 1
    for (int p = 0; p < 11; ++p)
#pragma unroll 1
      for (int q = p + 1; q < 12; ++q) {
        const double g = PNP_A(p, q);
        if (g == 0) continue;
        const double app = PNP_A(p, p), aqq = PNP_A(q, q), h = 100 * fabs(g);
        if (fabs(app) + h == fabs(app) && fabs(aqq) + h == fabs(aqq)) {
          PNP_A(p, q) = 0, PNP_A(q, p) = 0;
          continue;
        }
        rotated = true;
        double t, cs, sn;
        pnp_rot(app, aqq, g, t, cs, sn);
        PNP_A(p, p) = app - t * g, PNP_A(q, q) = aqq + t * g, PNP_A(p, q) = 0, PNP_A(q, p) = 0;
#pragma unroll 1
        for (int k = 0; k < 12; ++k) {
          if (k != p && k != q) {
            const double u = PNP_A(k, p), v = PNP_A(k, q);
            const double n1 = cs * u - sn * v, n2 = sn * u + cs * v;
            PNP_A(k, p) = n1, PNP_A(p, k) = n1, PNP_A(k, q) = n2, PNP_A(q, k) = n2;
          }
          const double vp = PNP_V(p, k), vq = PNP_V(q, k);
          PNP_V(p, k) = cs * vp - sn * vq, PNP_V(q, k) = sn * vp + cs * vq;
        }
      }
    if (!rotated) break;
  }
  // the four smallest eigenvalues, smallest first (ties: the lower index)
  int e[4];
  {
    unsigned taken = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      int best = -1;
      double bv = 0;
#pragma unroll 1
      for (int k = 0; k < 12; ++k) {
        const double v = PNP_A(k, k);
        if (!((taken >> k) & 1) && (best < 0 || v < bv)) best = k, bv = v;
      }
      e[s] = best, taken |= 1u << best;
      PNP_TAP(s, bv)
    }
  }
  // ---- compute_L_6x10 (differences of the control points' coordinates in each vector; slots 0..71 of the freed sA),
  // the matrix itself in slots 72..131, compute_rho
  constexpr int kA[6] = {0, 0, 0, 1, 1, 2}, kB[6] = {1, 2, 3, 2, 3, 3};  // the six pairs of control points
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 6; ++j) {
#pragma unroll
      for (int c = 0; c < 3; ++c) PNP_S((i * 6 + j) * 3 + c) = PNP_V(e[i], 3 * kA[j] + c) - PNP_V(e[i], 3 * kB[j] + c);
    }
  }
#define PNP_DOT(i, j, r) \
  ((PNP_S(((i) * 6 + (r)) * 3) * PNP_S(((j) * 6 + (r)) * 3) + PNP_S(((i) * 6 + (r)) * 3 + 1) * PNP_S(((j) * 6 + (r)) * 3 + 1)) + \
   PNP_S(((i) * 6 + (r)) * 3 + 2) * PNP_S(((j) * 6 + (r)) * 3 + 2))
#define PNP_L(r, c) PNP_S(72 + (r) * 10 + (c))
#pragma unroll 1
  for (int r = 0; r < 6; ++r) {
    PNP_L(r, 0) = PNP_DOT(0, 0, r);
    PNP_L(r, 1) = 2.0 * PNP_DOT(0, 1, r);
    PNP_L(r, 2) = PNP_DOT(1, 1, r);
    PNP_L(r, 3) = 2.0 * PNP_DOT(0, 2, r);
    PNP_L(r, 4) = 2.0 * PNP_DOT(1, 2, r);
    PNP_L(r, 5) = PNP_DOT(2, 2, r);
    PNP_L(r, 6) = 2.0 * PNP_DOT(0, 3, r);
    PNP_L(r, 7) = 2.0 * PNP_DOT(1, 3, r);
    PNP_L(r, 8) = 2.0 * PNP_DOT(2, 3, r);
    PNP_L(r, 9) = PNP_DOT(3, 3, r);
  }
  double rho[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const double d0 = co[kA[j]][0] - co[kB[j]][0], d1 = co[kA[j]][1] - co[kB[j]][1], d2 = co[kA[j]][2] - co[kB[j]][2];
    rho[j] = (d0 * d0 + d1 * d1) + d2 * d2;
    PNP_TAP(4 + j, rho[j])
  }
  // ---- the three initial guesses, gauss_newton, compute_R_and_t; the smallest reprojection error wins
  double best_err = 0;
#pragma unroll 1
  for (int variant = 1; variant <= 3; ++variant) {
    double betas[4] = {0, 0, 0, 0};
    if (variant == 1) {  // [B11 B12 B13 B14]
      double A[6][4], b[6], x[4];
#pragma unroll
      for (int r = 0; r < 6; ++r) A[r][0] = PNP_L(r, 0), A[r][1] = PNP_L(r, 1), A[r][2] = PNP_L(r, 3), A[r][3] = PNP_L(r, 6), b[r] = rho[r];
      pnp_lstsq6<4>(A, b, x);
      PNP_TAP(31, x[0]) PNP_TAP(32, x[1]) PNP_TAP(33, x[2]) PNP_TAP(34, x[3])
      const double sg = x[0] < 0 ? -1. : 1.;
      betas[0] = sqrt(sg * x[0]);
      betas[1] = sg * x[1] / betas[0], betas[2] = sg * x[2] / betas[0], betas[3] = sg * x[3] / betas[0];
    } else if (variant == 2) {  // [B11 B12 B22]
      double A[6][3], b[6], x[3];
#pragma unroll
      for (int r = 0; r < 6; ++r) A[r][0] = PNP_L(r, 0), A[r][1] = PNP_L(r, 1), A[r][2] = PNP_L(r, 2), b[r] = rho[r];
      pnp_lstsq6<3>(A, b, x);
      PNP_TAP(35, x[0]) PNP_TAP(36, x[1]) PNP_TAP(37, x[2])
      if (x[0] < 0)
        betas[0] = sqrt(-x[0]), betas[1] = x[2] < 0 ? sqrt(-x[2]) : 0.0;
      else
        betas[0] = sqrt(x[0]), betas[1] = x[2] > 0 ? sqrt(x[2]) : 0.0;
      if (x[1] < 0) betas[0] = -betas[0];
    } else {  // [B11 B12 B22 B13 B23]
      double A[6][5], b[6], x[5];
#pragma unroll
      for (int r = 0; r < 6; ++r) {
#pragma unroll
        for (int c = 0; c < 5; ++c) A[r][c] = PNP_L(r, c);
        b[r] = rho[r];
      }
      pnp_lstsq6<5>(A, b, x);
      PNP_TAP(38, x[0]) PNP_TAP(39, x[1]) PNP_TAP(40, x[2]) PNP_TAP(41, x[3]) PNP_TAP(42, x[4])
      if (x[0] < 0)
        betas[0] = sqrt(-x[0]), betas[1] = x[2] < 0 ? sqrt(-x[2]) : 0.0;
      else
        betas[0] = sqrt(x[0]), betas[1] = x[2] > 0 ? sqrt(x[2]) : 0.0;
      if (x[1] < 0) betas[0] = -betas[0];
      betas[2] = x[3] / betas[0];
    }
    PNP_TAP(10 + 4 * (variant - 1), betas[0]) PNP_TAP(11 + 4 * (variant - 1), betas[1])
    PNP_TAP(12 + 4 * (variant - 1), betas[2]) PNP_TAP(13 + 4 * (variant - 1), betas[3])
#pragma unroll 1
    for (int it = 0; it < 5; ++it) {  // gauss_newton
      double A[6][4], b[6], x[4];
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        double L[10];
#pragma unroll
        for (int c = 0; c < 10; ++c) L[c] = PNP_L(r, c);
        A[r][0] = ((2 * L[0] * betas[0] + L[1] * betas[1]) + L[3] * betas[2]) + L[6] * betas[3];
        A[r][1] = ((L[1] * betas[0] + 2 * L[2] * betas[1]) + L[4] * betas[2]) + L[7] * betas[3];
        A[r][2] = ((L[3] * betas[0] + L[4] * betas[1]) + 2 * L[5] * betas[2]) + L[8] * betas[3];
        A[r][3] = ((L[6] * betas[0] + L[7] * betas[1]) + L[8] * betas[2]) + 2 * L[9] * betas[3];
        b[r] = rho[r] - (((((((((L[0] * betas[0] * betas[0] + L[1] * betas[0] * betas[1]) + L[2] * betas[1] * betas[1]) +
                               L[3] * betas[0] * betas[2]) + L[4] * betas[1] * betas[2]) + L[5] * betas[2] * betas[2]) +
                            L[6] * betas[0] * betas[3]) + L[7] * betas[1] * betas[3]) + L[8] * betas[2] * betas[3]) +
                         L[9] * betas[3] * betas[3]);
      }
      pnp_lstsq6<4>(A, b, x);
#pragma unroll
      for (int c = 0; c < 4; ++c) betas[c] += x[c];
    }
    // compute_ccs, compute_pcs on the fly, solve_for_sign
    double cc[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        cc[j][c] = ((betas[0] * PNP_V(e[0], 3 * j + c) + betas[1] * PNP_V(e[1], 3 * j + c)) + betas[2] * PNP_V(e[2], 3 * j + c)) +
                   betas[3] * PNP_V(e[3], 3 * j + c);
    {
      double a[4];
      pnp_alphas(F, Xc + 3 * idx[0], a);
      const double z0 = ((a[0] * cc[0][2] + a[1] * cc[1][2]) + a[2] * cc[2][2]) + a[3] * cc[3][2];
      PNP_TAP(24 + variant, z0)
      if (z0 < 0.0) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int c = 0; c < 3; ++c) cc[j][c] = -cc[j][c];
      }
    }
    // estimate_R_and_t
    double pc0[3] = {0, 0, 0}, pw0[3] = {0, 0, 0};
    for (int i = 0; i < cnt; ++i) {
      const float* X = Xc + 3 * idx[i];
      double a[4];
      pnp_alphas(F, X, a);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        pc0[c] += ((a[0] * cc[0][c] + a[1] * cc[1][c]) + a[2] * cc[2][c]) + a[3] * cc[3][c];
        pw0[c] += (double)X[c];
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) pc0[c] /= cnt, pw0[c] /= cnt;
    double B[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int i = 0; i < cnt; ++i) {
      const float* X = Xc + 3 * idx[i];
      double a[4];
      pnp_alphas(F, X, a);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double pc = (((a[0] * cc[0][r] + a[1] * cc[1][r]) + a[2] * cc[2][r]) + a[3] * cc[3][r]) - pc0[r];
#pragma unroll
        for (int c = 0; c < 3; ++c) B[r][c] += pc * ((double)X[c] - pw0[c]);
      }
    }
    double R[3][3], t[3];
    pnp_polar3(B, R);
    const double det = ((((R[0][0] * R[1][1] * R[2][2] + R[0][1] * R[1][2] * R[2][0]) + R[0][2] * R[1][0] * R[2][1]) -
                         R[0][2] * R[1][1] * R[2][0]) - R[0][1] * R[1][0] * R[2][2]) - R[0][0] * R[1][2] * R[2][1];
    PNP_TAP(27 + variant, det)
    if (det < 0) R[2][0] = -R[2][0], R[2][1] = -R[2][1], R[2][2] = -R[2][2];
#pragma unroll
    for (int r = 0; r < 3; ++r) t[r] = pc0[r] - ((R[r][0] * pw0[0] + R[r][1] * pw0[1]) + R[r][2] * pw0[2]);
    // reprojection_error
    double sum = 0;
    for (int i = 0; i < cnt; ++i) {
      const int g = idx[i];
      double ue, ve;
      if constexpr (RIG)
        pnp_project_rig(*G.rig, Cam[g], R, t, Xc + 3 * g, ue, ve);
      else
        pnp_project(C, R, t, Xc + 3 * g, ue, ve);
      const double du = (double)Uc[2 * g] - ue, dv = (double)Uc[2 * g + 1] - ve;
      sum += sqrt(du * du + dv * dv);
    }
    const double err = sum / cnt;
    PNP_TAP(21 + variant, err)
    if (variant == 1 || err < best_err) {
      best_err = err;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        tout[r] = t[r];
#pragma unroll
        for (int c = 0; c < 3; ++c) Rout[r][c] = R[r][c];
      }
    }
  }
#undef PNP_DOT
#undef PNP_L
}

// the rectified configuration
PNP_DEV void pnp_epnp(const PnpCandDev& C, const float* __restrict__ Xw, const float* __restrict__ uv,
                                      const int* __restrict__ idx, int cnt, double* sA, double* sV, int lane,
                                      double (&Rout)[3][3], double (&tout)[3]) {
  pnp_epnp_t<false>(C, PnpRigArgs{nullptr, nullptr, nullptr}, Xw, uv, idx, cnt, sA, sV, lane, Rout, tout);
}

// CheckInliers over all n correspondences of the candidate; a pose that is not finite has none.  RIG: through the rig
// Getuv, where a pixel that is not finite fails error2 < mvMaxError like any other outlier.
template <bool RIG>
PNP_DEV int pnp_check_inliers_t(const PnpCandDev& C, const PnpRigArgs& G, const float* __restrict__ Xw,
                                                 const float* __restrict__ uv, const float* __restrict__ max_err,
                                                 const double (&R)[3][3], const double (&t)[3],
                                                 unsigned long long* __restrict__ mask) {
  bool fin = true;
#pragma unroll
  for (int r = 0; r < 3; ++r) fin = fin && std::isfinite(t[r]) && std::isfinite(R[r][0]) && std::isfinite(R[r][1]) && std::isfinite(R[r][2]);
  int count = 0;
  for (int w = 0; w < C.words; ++w) {
    unsigned long long bits = 0;
    const int end = C.n - 64 * w < 64 ? C.n - 64 * w : 64;
    for (int b = 0; fin && b < end; ++b) {
      const int g = C.off + 64 * w + b;
      double ue, ve;
      if constexpr (RIG)
        pnp_project_rig(*G.rig, G.cam_of[g], R, t, Xw + 3 * (size_t)g, ue, ve);
      else
        pnp_project(C, R, t, Xw + 3 * (size_t)g, ue, ve);
      const float dx = (float)((double)uv[2 * (size_t)g] - ue), dy = (float)((double)uv[2 * (size_t)g + 1] - ve);
      const float err2 = dx * dx + dy * dy;
      if (err2 < max_err[g]) bits |= 1ull << b, ++count;
    }
    mask[w] = bits;
  }
  return count;
}

PNP_DEV int pnp_check_inliers(const PnpCandDev& C, const float* __restrict__ Xw,
                                                 const float* __restrict__ uv, const float* __restrict__ max_err,
                                                 const double (&R)[3][3], const double (&t)[3],
                                                 unsigned long long* __restrict__ mask) {
  return pnp_check_inliers_t<false>(C, PnpRigArgs{nullptr, nullptr, nullptr}, Xw, uv, max_err, R, t, mask);
}

PNP_DEV void pnp_store_pose(const double (&R)[3][3], const double (&t)[3], double* __restrict__ Rt) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) Rt[3 * r + c] = R[r][c];
    Rt[9 + r] = t[r];
  }
}

}  // namespace vieo
