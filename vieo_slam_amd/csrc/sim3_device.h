// sim3_device.h -- the Sim3 algebra of the pose graph (pose_graph.hip): exp, log, product, inverse, map, as g2o's
// types/sim3.h states them, in FP64.  All four eps = 1e-5 branches of exp and of log are kept as they are there (C = 1
// for |sigma| < eps, R = I + Omega + Omega^2 / 2 for theta < eps, omega = 0.5 deltaR for d > 1 - eps and
// theta / (2 sqrt(1 - d^2)) deltaR otherwise); matrix <-> quaternion and the rotation of a vector are Eigen's; the 3 x 3
// solve of log is the closed form (adjugate / determinant).  Plain functions on plain doubles, host and device, so a
// host program can run them too.
#pragma once
#include <cmath>

#ifdef __HIPCC__
#define VIEO_S3_HD __host__ __device__ inline
#else
#define VIEO_S3_HD inline
#endif

// A test program may define S3_TAP(slot, value) before including this file to record the values that decide the
// branches: 0 / 1 the branch (0: trace > 0, 1 + i else) and the trace of s3_mat_to_quat, 2 / 3 theta < eps and theta of
// s3_exp, 4 its |sigma| < eps, 5 / 6 d > 1 - eps and d of s3_log, 7 / 8 its |sigma| < eps and sigma, 9 / 10 theta < 1e-5
// and theta of s3o_inc_small (sim3_optimize_device.h).  Empty in the library.
#ifndef S3_TAP
#define S3_TAP(slot, value)
#endif

namespace vieo {

struct Sim3 {  // the layout of vieo_sim3
  double q[4];  // x, y, z, w
  double t[3];
  double s;
};

VIEO_S3_HD void s3_quat_to_mat(const double* q, double R[9]) {  // Eigen::QuaternionBase::toRotationMatrix
  const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
  const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
  const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
  const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
  R[0] = 1 - (tyy + tzz), R[1] = txy - twz, R[2] = txz + twy;
  R[3] = txy + twz, R[4] = 1 - (txx + tzz), R[5] = tyz - twx;
  R[6] = txz - twy, R[7] = tyz + twx, R[8] = 1 - (txx + tyy);
}

VIEO_S3_HD void s3_mat_to_quat(const double R[9], double* q) {  // Eigen: quaternionbase_assign_impl<Other, 3, 3>
  double t = R[0] + R[4] + R[8];
  S3_TAP(1, t)
  if (t > 0) {
    S3_TAP(0, 0.0)
    t = sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (R[7] - R[5]) * t;
    q[1] = (R[2] - R[6]) * t;
    q[2] = (R[3] - R[1]) * t;
  } else {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[4 * i]) i = 2;
    S3_TAP(0, 1.0 + i)
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0);
    q[i] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (R[3 * k + j] - R[3 * j + k]) * t;
    q[j] = (R[3 * j + i] + R[3 * i + j]) * t;
    q[k] = (R[3 * k + i] + R[3 * i + k]) * t;
  }
}

VIEO_S3_HD void s3_quat_mul(const double* a, const double* b, double* o) {  // Eigen: quat_product
  const double w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
  const double x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  const double y = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  const double z = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
  o[0] = x, o[1] = y, o[2] = z, o[3] = w;
}

VIEO_S3_HD void s3_quat_rot(const double* q, const double* v, double* o) {  // Eigen: _transformVector
  double ux = q[1] * v[2] - q[2] * v[1], uy = q[2] * v[0] - q[0] * v[2], uz = q[0] * v[1] - q[1] * v[0];
  ux += ux, uy += uy, uz += uz;
  const double cx = q[1] * uz - q[2] * uy, cy = q[2] * ux - q[0] * uz, cz = q[0] * uy - q[1] * ux;
  o[0] = v[0] + q[3] * ux + cx, o[1] = v[1] + q[3] * uy + cy, o[2] = v[2] + q[3] * uz + cz;
}

VIEO_S3_HD Sim3 s3_identity() {
  Sim3 S;
  S.q[0] = S.q[1] = S.q[2] = 0, S.q[3] = 1, S.t[0] = S.t[1] = S.t[2] = 0, S.s = 1;
  return S;
}

VIEO_S3_HD Sim3 s3_mul(const Sim3& a, const Sim3& b) {  // sim3.h:245-251
  Sim3 o;
  s3_quat_mul(a.q, b.q, o.q);
  double r[3];
  s3_quat_rot(a.q, b.t, r);
  for (int i = 0; i < 3; i++) o.t[i] = a.s * r[i] + a.t[i];
  o.s = a.s * b.s;
  return o;
}

VIEO_S3_HD Sim3 s3_inverse(const Sim3& a) {  // sim3.h:218-221
  Sim3 o;
  o.q[0] = -a.q[0], o.q[1] = -a.q[1], o.q[2] = -a.q[2], o.q[3] = a.q[3];
  const double m = -1. / a.s;
  const double v[3] = {m * a.t[0], m * a.t[1], m * a.t[2]};
  s3_quat_rot(o.q, v, o.t);
  o.s = 1. / a.s;
  return o;
}

VIEO_S3_HD void s3_map(const Sim3& a, const double* p, double* o) {  // sim3.h:138-140
  double r[3];
  s3_quat_rot(a.q, p, r);
  for (int i = 0; i < 3; i++) o[i] = a.s * r[i] + a.t[i];
}

// W = A Omega + B Omega^2 + C I  (Omega = skew(w))
VIEO_S3_HD void s3_w_matrix(const double* w, double A, double B, double C, double W[9]) {
  const double O[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double o2 = 0;
      for (int k = 0; k < 3; k++) o2 += O[3 * i + k] * O[3 * k + j];
      W[3 * i + j] = A * O[3 * i + j] + B * o2 + (i == j ? C : 0.0);
    }
}

VIEO_S3_HD Sim3 s3_exp(const double* u) {  // sim3.h:61-136
  const double* omega = u;
  const double* upsilon = u + 3;
  const double sigma = u[6];
  const double theta = sqrt(omega[0] * omega[0] + omega[1] * omega[1] + omega[2] * omega[2]);
  const double O[9] = {0, -omega[2], omega[1], omega[2], 0, -omega[0], -omega[1], omega[0], 0};
  double O2[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double a = 0;
      for (int k = 0; k < 3; k++) a += O[3 * i + k] * O[3 * k + j];
      O2[3 * i + j] = a;
    }
  Sim3 S;
  S.s = exp(sigma);
  const double eps = 0.00001;
  double A, B, C, R[9];
  const bool small_theta = theta < eps;
  S3_TAP(2, small_theta ? 1.0 : 0.0) S3_TAP(3, theta) S3_TAP(4, fabs(sigma) < eps ? 1.0 : 0.0)
  if (small_theta) {
    for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + O[i] + O2[i] / 2;
  } else {
    const double a = sin(theta) / theta, b = (1 - cos(theta)) / (theta * theta);
    for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + a * O[i] + b * O2[i];
  }
  if (fabs(sigma) < eps) {
    C = 1;
    if (small_theta) {
      A = 1. / 2.;
      B = 1. / 6.;
    } else {
      const double theta2 = theta * theta;
      A = (1 - cos(theta)) / theta2;
      B = (theta - sin(theta)) / (theta2 * theta);
    }
  } else {
    C = (S.s - 1) / sigma;
    if (small_theta) {
      const double sigma2 = sigma * sigma;
      A = ((sigma - 1) * S.s + 1) / sigma2;
      B = ((0.5 * sigma2 - sigma + 1) * S.s - 1) / (sigma2 * sigma);
    } else {
      const double a = S.s * sin(theta), b = S.s * cos(theta);
      const double theta2 = theta * theta, sigma2 = sigma * sigma;
      const double c = theta2 + sigma2;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
    }
  }
  s3_mat_to_quat(R, S.q);
  for (int i = 0; i < 3; i++) {
    double a = 0;
    for (int j = 0; j < 3; j++) a += (A * O[3 * i + j] + B * O2[3 * i + j] + (i == j ? C : 0.0)) * upsilon[j];
    S.t[i] = a;
  }
  return S;
}

VIEO_S3_HD void s3_log(const Sim3& S, double* res) {  // sim3.h:143-216
  const double sigma = log(S.s);
  double R[9];
  s3_quat_to_mat(S.q, R);
  const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
  const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
  const double eps = 0.00001;
  double omega[3], A, B, C;
  const bool near_identity = d > 1 - eps;
  S3_TAP(5, near_identity ? 1.0 : 0.0) S3_TAP(6, d) S3_TAP(7, fabs(sigma) < eps ? 1.0 : 0.0) S3_TAP(8, sigma)
  double theta = 0;
  if (near_identity) {
    for (int i = 0; i < 3; i++) omega[i] = 0.5 * dR[i];
  } else {
    theta = acos(d);
    const double f = theta / (2 * sqrt(1 - d * d));
    for (int i = 0; i < 3; i++) omega[i] = f * dR[i];
  }
  if (fabs(sigma) < eps) {
    C = 1;
    if (near_identity) {
      A = 1. / 2.;
      B = 1. / 6.;
    } else {
      const double theta2 = theta * theta;
      A = (1 - cos(theta)) / theta2;
      B = (theta - sin(theta)) / (theta2 * theta);
    }
  } else {
    C = (S.s - 1) / sigma;
    if (near_identity) {
      const double sigma2 = sigma * sigma;
      A = ((sigma - 1) * S.s + 1) / sigma2;
      B = ((0.5 * sigma2 - sigma + 1) * S.s - 1) / (sigma2 * sigma);
    } else {
      const double theta2 = theta * theta;
      const double a = S.s * sin(theta), b = S.s * cos(theta);
      const double c = theta2 + sigma * sigma;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
    }
  }
  double W[9];
  s3_w_matrix(omega, A, B, C, W);
  // upsilon = W^-1 t, closed form
  const double c00 = W[4] * W[8] - W[5] * W[7], c01 = W[5] * W[6] - W[3] * W[8], c02 = W[3] * W[7] - W[4] * W[6];
  const double c10 = W[2] * W[7] - W[1] * W[8], c11 = W[0] * W[8] - W[2] * W[6], c12 = W[1] * W[6] - W[0] * W[7];
  const double c20 = W[1] * W[5] - W[2] * W[4], c21 = W[2] * W[3] - W[0] * W[5], c22 = W[0] * W[4] - W[1] * W[3];
  const double det = W[0] * c00 + W[1] * c01 + W[2] * c02;
  res[0] = omega[0], res[1] = omega[1], res[2] = omega[2];
  res[3] = (c00 * S.t[0] + c10 * S.t[1] + c20 * S.t[2]) / det;
  res[4] = (c01 * S.t[0] + c11 * S.t[1] + c21 * S.t[2]) / det;
  res[5] = (c02 * S.t[0] + c12 * S.t[1] + c22 * S.t[2]) / det;
  res[6] = sigma;
}

// EdgeSim3::computeError: log(C * Si * Sj^-1)
VIEO_S3_HD void s3_edge_error(const Sim3& C, const Sim3& Si, const Sim3& Sj, double* e) {
  s3_log(s3_mul(s3_mul(C, Si), s3_inverse(Sj)), e);
}

}  // namespace vieo
