// imu_init_device.h -- the lane functions of IMUInitialization::TryInitVIO (imu_init.hip; reference
// src/Odom/IMUInitialization.cpp:1068-1480, USE_FAST_IMU_INIT undefined): the gyro-bias edge (EdgeGyrBias,
// src/Odom/g2otypes.h:940-973) with the Gauss-Newton step of OptimizeInitialGyroBias (include/Optimizer.h:820-892), the
// rows of the two least-squares problems (:1154-1195, :1263-1296), a one-sided (Hestenes) Jacobi SVD that solves them and
// returns their singular values, the gravity frame RwI and the closed forms of the map update (:1393-1459).  Everything
// that runs on a wavefront is templated on a functor `Lanes`:
//   L.run<N>(f, out)  f(lane, n_lanes, part[N]) on every lane, out[N] = the sum over the lanes, the same on all of them
//   L.sync()          what the lanes wrote into the row matrix is visible to all of them
// so the file also compiles as ordinary C++, where a functor of 1 or 64 lanes runs the same code on a host
// (tests/emul/imu_init_emul.cc).  On the device the SO(3) closed forms are imu_device.h's; a host build supplies the same
// functions (Qd, q_norm, q_mul, q_conj, q_to_R, R_to_q, so3_exp_q, so3_log_q, so3_JrInv_d, mm3, mv3) before including
// this file.
//
// Why Jacobi and not the normal equations: the singular values are outputs, and the normal equations would square a
// condition number that reaches 6e3 on the synthetic sequences.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#include "imu_device.h"
#define VIEO_II_FN __device__ __forceinline__
#define VIEO_II_CALL __device__ __noinline__  // the big lane functions: one body each, called
#else
#define VIEO_II_FN static inline
#define VIEO_II_CALL static inline
#endif

namespace vieo {

struct IiSeq {  // one sequence as steps 1-4 read it: the snapshot of n key frames
  const double* Twc;           // [n][12] rows of (Rwc | pwc)
  const vieo_imu_preint* pre;  // [n] entry i: the interval (i - 1) -> i; entry 0 is not read
  const double* prv;           // [n][81] mSigmaijPRV of the same intervals (step 1 only)
  int n;
  double Rcb[9], pcb[3], G;
};

VIEO_II_FN void ii_Rwc(const double* T, double* R) {
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) R[3 * r + c] = T[4 * r + c];
}

// Matrix3d::inverse() of a 3 x 3 block with leading dimension ld (Eigen: cofactors over the determinant)
VIEO_II_FN void ii_inv3(const double* S, int ld, double* W) {
  const double a = S[0], b = S[1], c = S[2], d = S[ld], e = S[ld + 1], f = S[ld + 2], g = S[2 * ld], h = S[2 * ld + 1],
               i = S[2 * ld + 2];
  const double c00 = e * i - f * h, c10 = f * g - d * i, c20 = d * h - e * g;
  const double inv = 1.0 / (a * c00 + b * c10 + c * c20);
  W[0] = c00 * inv, W[1] = (c * h - b * i) * inv, W[2] = (b * f - c * e) * inv;
  W[3] = c10 * inv, W[4] = (a * i - c * g) * inv, W[5] = (c * d - a * f) * inv;
  W[6] = c20 * inv, W[7] = (b * g - a * h) * inv, W[8] = (a * e - b * d) * inv;
}

// EdgeGyrBias at bg = 0 for key frame i >= 1 (the edge between key frames i - 1 and i): e = Log(dRij^T Rwbi^T Rwbj),
// J = -JrInv(e) Exp(-e) Jr(0) JgR with Jr(0) = I, W = (Phi block of mSigmaijPRV)^-1
VIEO_II_CALL void ii_gyro_edge(const double* Rcb, const double* Twc_i, const double* Twc_j, const vieo_imu_preint& P,
                               const double* prv, double* e, double* J, double* W) {
  double Rc[9], Rwbi[9], Rwbj[9], A[9], M[9];
  ii_Rwc(Twc_i, Rc);
  mm3(Rc, Rcb, Rwbi);
  ii_Rwc(Twc_j, Rc);
  mm3(Rc, Rcb, Rwbj);
  for (int r = 0; r < 3; r++)  // A = dRij^T Rwbi^T = (Rwbi dRij)^T
    for (int c = 0; c < 3; c++)
      A[3 * r + c] = (Rwbi[3 * c] * P.Rij[r] + Rwbi[3 * c + 1] * P.Rij[3 + r]) + Rwbi[3 * c + 2] * P.Rij[6 + r];
  mm3(A, Rwbj, M);
  so3_log_q(R_to_q(M), e);
  double JrInv[9], E[9], T[9];
  so3_JrInv_d(e, JrInv);
  const double me[3] = {-e[0], -e[1], -e[2]};
  q_to_R(so3_exp_q(me), E);
  mm3(JrInv, E, T);
  mm3(T, P.JgR, J);
  for (int k = 0; k < 9; k++) J[k] = -J[k];
  ii_inv3(prv + 3 * 9 + 3, 9, W);
}

// H x = b for the symmetric 3 x 3 H = (h00 h01 h02 h11 h12 h22) by LDL^T; false (x = 0) when a pivot is not positive
VIEO_II_FN bool ii_ldlt3(const double* h, const double* b, double* x) {
  x[0] = x[1] = x[2] = 0;
  const double d0 = h[0];
  if (!(d0 > 0)) return false;
  const double l10 = h[1] / d0, l20 = h[2] / d0;
  const double d1 = h[3] - l10 * h[1];
  if (!(d1 > 0)) return false;
  const double l21 = (h[4] - l20 * h[1]) / d1;
  const double d2 = h[5] - l20 * h[2] - l21 * (l21 * d1);
  if (!(d2 > 0)) return false;
  const double y0 = b[0], y1 = b[1] - l10 * y0, y2 = b[2] - l20 * y0 - l21 * y1;
  const double z2 = y2 / d2, z1 = y1 / d1 - l21 * z2, z0 = y0 / d0 - l10 * z1 - l20 * z2;
  x[0] = z0, x[1] = z1, x[2] = z2;
  return true;
}

// Step 1: one Gauss-Newton step from bg = 0; the lanes stride over the edges
template <class Lanes>
VIEO_II_FN void ii_gyro_step(Lanes& L, const IiSeq& S, double* bg, int* n_eq) {
  double acc[10];
  L.template run<10>(
      [&](int lane, int nl, double* part) {
        for (int k = 0; k < 10; k++) part[k] = 0;
        for (int i = 1 + lane; i < S.n; i += nl) {
          const vieo_imu_preint& P = S.pre[i];
          if (P.dt == 0) continue;
          double e[3], J[9], W[9], WJ[9], We[3];
          ii_gyro_edge(S.Rcb, S.Twc + 12 * (size_t)(i - 1), S.Twc + 12 * (size_t)i, P, S.prv + 81 * (size_t)i, e, J, W);
          mm3(W, J, WJ);
          mv3(W, e, We);
          int k = 0;
          for (int a = 0; a < 3; a++)
            for (int b = a; b < 3; b++, k++) part[k] += (J[a] * WJ[b] + J[3 + a] * WJ[3 + b]) + J[6 + a] * WJ[6 + b];
          for (int a = 0; a < 3; a++) part[6 + a] -= (J[a] * We[0] + J[3 + a] * We[1]) + J[6 + a] * We[2];
          part[9] += 1;
        }
      },
      acc);
  *n_eq = (int)acc[9];
  bg[0] = bg[1] = bg[2] = 0;
  if (*n_eq >= 1) ii_ldlt3(acc, acc + 6, bg);
}

// What the rows of both problems share for the triple (i, i + 1, i + 2): lambda, beta and gamma (:1186-1190); false when
// one of the two intervals has dt == 0
VIEO_II_CALL bool ii_triple(const IiSeq& S, int i, double* lam, double* beta, double* gam, double* R1b, double* R2b) {
  const vieo_imu_preint &P2 = S.pre[i + 1], &P3 = S.pre[i + 2];
  const double dt12 = P2.dt, dt23 = P3.dt;
  if (dt12 == 0 || dt23 == 0) return false;
  const double *T1 = S.Twc + 12 * (size_t)i, *T2 = T1 + 12, *T3 = T1 + 24;
  double R1[9], R2[9], R3[9], D12[9], D32[9], a[3], b[3], c[3], d[3], f[3];
  ii_Rwc(T1, R1), ii_Rwc(T2, R2), ii_Rwc(T3, R3);
  for (int k = 0; k < 3; k++) lam[k] = (T2[4 * k + 3] - T1[4 * k + 3]) * dt23 + (T2[4 * k + 3] - T3[4 * k + 3]) * dt12;
  *beta = (dt12 * dt12 * dt23 + dt12 * dt23 * dt23) / 2;
  for (int k = 0; k < 9; k++) D12[k] = R1[k] - R2[k], D32[k] = R3[k] - R2[k];
  mm3(R1, S.Rcb, R1b);
  mm3(R2, S.Rcb, R2b);
  mv3(D12, S.pcb, a);
  mv3(D32, S.pcb, b);
  mv3(R2b, P3.pij, c);
  mv3(R1b, P2.vij, d);
  mv3(R1b, P2.pij, f);
  for (int k = 0; k < 3; k++) gam[k] = a[k] * dt23 + b[k] * dt12 - c[k] * dt12 - d[k] * (dt12 * dt23) + f[k] * dt23;
  return true;
}

// The row matrix M is column-major with leading dimension ld >= 3 (n - 2): column c of row r at M[c * ld + r]; the
// right-hand side is the column behind the unknowns.  A skipped triple leaves three zero rows.
// Step 3: [lambda | beta I3 | gamma]; returns the number of valid triples
template <class Lanes>
VIEO_II_FN int ii_fill_first(Lanes& L, const IiSeq& S, double* M, int ld) {
  double cnt;
  L.template run<1>(
      [&](int lane, int nl, double* part) {
        part[0] = 0;
        for (int i = lane; i < S.n - 2; i += nl) {
          double lam[3], beta, gam[3], R1b[9], R2b[9];
          const bool ok = ii_triple(S, i, lam, &beta, gam, R1b, R2b);
          for (int r = 0; r < 3; r++) {
            double* row = M + 3 * i + r;
            row[0] = ok ? lam[r] : 0;
            for (int c = 0; c < 3; c++) row[(1 + c) * ld] = ok && c == r ? beta : 0;
            row[4 * ld] = ok ? gam[r] : 0;
          }
          part[0] += ok ? 1 : 0;
        }
      },
      &cnt);
  L.sync();
  return (int)cnt;
}

// Step 4: [lambda | phi(:, 0:2) | zeta | psi] with phi = -beta RwI [GI]x (the reference's sign), zeta with Jav12 (the
// reference's comment: the paper writes Jav23), psi = gamma - beta RwI GI
template <class Lanes>
VIEO_II_FN void ii_fill_second(Lanes& L, const IiSeq& S, const double* RwI, double* M, int ld) {
  double unused;
  L.template run<1>(
      [&](int lane, int nl, double* part) {
        part[0] = 0;
        for (int i = lane; i < S.n - 2; i += nl) {
          double lam[3], beta, gam[3], R1b[9], R2b[9], Z[9], Z1[9], Z2[9];
          const bool ok = ii_triple(S, i, lam, &beta, gam, R1b, R2b);
          if (ok) {
            const vieo_imu_preint &P2 = S.pre[i + 1], &P3 = S.pre[i + 2];
            const double dt12 = P2.dt, dt23 = P3.dt;
            mm3(R2b, P3.Jap, Z);
            mm3(R1b, P2.Jav, Z1);
            mm3(R1b, P2.Jap, Z2);
            for (int k = 0; k < 9; k++) Z[k] = Z[k] * dt12 + Z1[k] * (dt12 * dt23) - Z2[k] * dt23;
          }
          for (int r = 0; r < 3; r++) {
            double* row = M + 3 * i + r;
            row[0] = ok ? lam[r] : 0;
            row[ld] = ok ? -beta * (RwI[3 * r + 1] * S.G) : 0;
            row[2 * ld] = ok ? beta * (RwI[3 * r] * S.G) : 0;
            for (int c = 0; c < 3; c++) row[(3 + c) * ld] = ok ? Z[3 * r + c] : 0;
            row[6 * ld] = ok ? gam[r] - beta * (RwI[3 * r + 2] * S.G) : 0;
          }
        }
      },
      &unused);
  L.sync();
}

// min |M x - B| over x for the m x NC columns of M and B = column NC, by a one-sided Jacobi SVD: plane rotations from the
// right make the columns orthogonal (fixed cyclic pair order (0,1), (0,2), .., (NC-2,NC-1); a pair rotates when
// |a_p . a_q| > sqrt(m) eps |a_p| |a_q|, dgesvj's test), until a sweep rotates nothing or VIEO_IMU_INIT_MAX_SWEEPS are
// done.  The singular values are the column norms, V accumulates the rotations, B is never rotated:
// (U^T B)_k = (a_k . B) / w_k.  |w_k| < 1e-10 is raised by 1e-10 as the reference does before it divides (a zero column
// has (U^T B)_k = 0).  w comes back sorted descending; returns the sweeps.  M is overwritten.
template <int NC, class Lanes>
VIEO_II_FN int ii_jacobi_solve(Lanes& L, double* M, int ld, int m, double* x, double* w) {
  double V[NC][NC];
#pragma unroll
  for (int a = 0; a < NC; a++)
#pragma unroll
    for (int b = 0; b < NC; b++) V[a][b] = a == b ? 1.0 : 0.0;
  const double tol = sqrt((double)m) * DBL_EPSILON;
  int sweeps = 0;
  while (sweeps < VIEO_IMU_INIT_MAX_SWEEPS) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < NC - 1; p++) {
#pragma unroll
      for (int q = p + 1; q < NC; q++) {
        double* ap = M + p * ld;
        double* aq = M + q * ld;
        double d[3];
        L.template run<3>(
            [&](int lane, int nl, double* part) {
              double a = 0, b = 0, g = 0;
              for (int r = lane; r < m; r += nl) {
                const double u = ap[r], v = aq[r];
                a += u * u, b += v * v, g += u * v;
              }
              part[0] = a, part[1] = b, part[2] = g;
            },
            d);
        if (d[2] == 0 || !(fabs(d[2]) > tol * sqrt(d[0] * d[1]))) continue;
        rotated = true;
        const double zeta = (d[1] - d[0]) / (2 * d[2]);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1 + zeta * zeta));
        const double c = 1.0 / sqrt(1 + t * t), s = c * t;
        double unused;
        L.template run<1>(
            [&](int lane, int nl, double* part) {
              part[0] = 0;
              for (int r = lane; r < m; r += nl) {
                const double u = ap[r], v = aq[r];
                ap[r] = c * u - s * v, aq[r] = s * u + c * v;
              }
            },
            &unused);
        L.sync();
#pragma unroll
        for (int k = 0; k < NC; k++) {
          const double u = V[k][p], v = V[k][q];
          V[k][p] = c * u - s * v, V[k][q] = s * u + c * v;
        }
      }
    }
    sweeps++;
    if (!rotated) break;
  }
  double nd[2 * NC];
  L.template run<2 * NC>(
      [&](int lane, int nl, double* part) {
#pragma unroll
        for (int k = 0; k < 2 * NC; k++) part[k] = 0;
        for (int r = lane; r < m; r += nl) {
          const double b = M[NC * ld + r];
#pragma unroll
          for (int k = 0; k < NC; k++) {
            const double u = M[k * ld + r];
            part[k] += u * u, part[NC + k] += u * b;
          }
        }
      },
      nd);
  // the solution in the rotated basis: y_k = (U^T B)_k / w_k
  double y[NC];
#pragma unroll
  for (int k = 0; k < NC; k++) {
    const double wk = sqrt(nd[k]);
    const double utb = wk > 0 ? nd[NC + k] / wk : 0;
    double wr = wk;
    if (fabs(wr) < 1e-10) wr += 1e-10;
    w[k] = wr;
    y[k] = utb / wr;
  }
  // One step of refinement there.  The sweeps leave the columns orthogonal to sqrt(m) eps only, and what is left couples
  // the directions: a direction of small w_k picks up (a_j . a_k) y_j / w_k^2 from one of large y_j -- 1e-13 of s* on 64
  // triples of condition 9, forty times the error of a bidiagonalising SVD.  y += D^-1 A'^T (B - A' y) with the rotated
  // columns A' takes the coupling out to second order.  A direction the rule raised is left as the rule made it.
  double corr[NC];
  L.template run<NC>(
      [&](int lane, int nl, double* part) {
#pragma unroll
        for (int k = 0; k < NC; k++) part[k] = 0;
        for (int r = lane; r < m; r += nl) {
          double a[NC], res = M[NC * ld + r];
#pragma unroll
          for (int k = 0; k < NC; k++) a[k] = M[k * ld + r], res -= a[k] * y[k];
#pragma unroll
          for (int k = 0; k < NC; k++) part[k] += a[k] * res;
        }
      },
      corr);
#pragma unroll
  for (int k = 0; k < NC; k++)
    if (nd[k] > 0 && !(sqrt(nd[k]) < 1e-10)) y[k] += corr[k] / nd[k];
#pragma unroll
  for (int k = 0; k < NC; k++) x[k] = 0;
#pragma unroll
  for (int k = 0; k < NC; k++)
#pragma unroll
    for (int a = 0; a < NC; a++) x[a] += V[a][k] * y[k];
#pragma unroll
  for (int a = 0; a < NC - 1; a++)  // descending (compile-time indices: the values stay in registers)
#pragma unroll
    for (int b = 0; b < NC - 1 - a; b++)
      if (w[b] < w[b + 1]) {
        const double t = w[b];
        w[b] = w[b + 1], w[b + 1] = t;
      }
  return sweeps;
}

// gwn = gw* / |gw*|, vhat = gI x gwn / |gI x gwn|, theta = atan2(|gI x gwn|, gI . gwn), RwI = Exp(vhat theta) with
// gI = (0, 0, 1); false where TryInitVIO would divide by zero (the guard of InitIMU:712-719)
VIEO_II_FN bool ii_gravity_frame(const double* gws, double* RwI) {
  const double n = sqrt((gws[0] * gws[0] + gws[1] * gws[1]) + gws[2] * gws[2]);
  if (!(n > 0)) return false;
  const double g[3] = {gws[0] / n, gws[1] / n, gws[2] / n};
  const double cx = -g[1], cy = g[0];
  const double nc = sqrt(cx * cx + cy * cy);
  if (!(nc > 0)) return false;
  const double theta = atan2(nc, g[2]);
  const double v[3] = {cx / nc * theta, cy / nc * theta, 0};
  q_to_R(so3_exp_q(v), RwI);
  return true;
}

// Steps 3 and 4 on the re-integrated intervals; R.bg / R.n_eq_gyro are the caller's.  M: 7 columns of ld doubles.
template <class Lanes>
VIEO_II_FN void ii_solve(Lanes& L, const IiSeq& S, double* M, int ld, vieo_imu_init_result& R) {
  const int m = 3 * (S.n - 2);
  R.n_eq = ii_fill_first(L, S, M, ld);
  if (R.n_eq < 4) {
    R.status = VIEO_IMU_INIT_FEW_EQUATIONS;
    return;
  }
  double x[4];
  R.sweeps[0] = ii_jacobi_solve<4>(L, M, ld, m, x, R.w);
  R.s_star = x[0];
  for (int k = 0; k < 3; k++) R.gw_star[k] = x[1 + k];
  if (!ii_gravity_frame(R.gw_star, R.RwI)) {
    R.status = VIEO_IMU_INIT_DEGENERATE_GRAVITY;
    return;
  }
  L.sync();
  ii_fill_second(L, S, R.RwI, M, ld);
  double y[6];
  R.sweeps[1] = ii_jacobi_solve<6>(L, M, ld, m, y, R.w2);
  R.s = y[0], R.dtheta[0] = y[1], R.dtheta[1] = y[2];
  for (int k = 0; k < 3; k++) R.ba[k] = y[3 + k];
  const double dth[3] = {y[1], y[2], 0};
  double E[9];
  q_to_R(so3_exp_q(dth), E);
  mm3(R.RwI, E, R.RwI_opt);
  for (int k = 0; k < 3; k++) R.gw[k] = R.RwI_opt[3 * k + 2] * S.G;
  R.status = VIEO_IMU_INIT_OK;
}

// ---- step 5, per key frame (:1393-1459)
// Tcw = (Rwc^T | -s Rwc^T pwc)
VIEO_II_FN void ii_scaled_Tcw(const double* Twc, double s, double* Tcw) {
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) Tcw[4 * r + c] = Twc[4 * c + r];
    const double t = -((Twc[r] * Twc[3] + Twc[4 + r] * Twc[7]) + Twc[8 + r] * Twc[11]);
    Tcw[4 * r + 3] = t * s;
  }
}
// pwb = s pwc + Rwc pcb, Rwb = Rwc Rcb (as a unit quaternion w, x, y, z); Rwb[9] comes back too
VIEO_II_FN void ii_nav_pose(const double* Twc, const double* Rcb, const double* pcb, double s, double* p, double* q,
                            double* Rwb) {
  double Rc[9], r[3];
  ii_Rwc(Twc, Rc);
  mv3(Rc, pcb, r);
  for (int k = 0; k < 3; k++) p[k] = s * Twc[4 * k + 3] + r[k];
  mm3(Rc, Rcb, Rwb);
  const Qd Q = R_to_q(Rwb);
  q[0] = Q.w, q[1] = Q.x, q[2] = Q.y, q[3] = Q.z;
}
// vwb_i = -1/dt (s (pwc_i - pwc_j) + (Rwc_i - Rwc_j) pcb + dt^2/2 gw + Rwc_i Rcb dp), (dt, dp) of the interval i -> j
// re-integrated with (bg*, ba*)
VIEO_II_FN void ii_velocity(const double* Twc_i, const double* Twc_j, const double* Rcb, const double* pcb, double s,
                            const double* gw, double dt, const double* dp, double* v) {
  double Ri[9], Rj[9], D[9], Rb[9], a[3], b[3];
  ii_Rwc(Twc_i, Ri), ii_Rwc(Twc_j, Rj);
  for (int k = 0; k < 9; k++) D[k] = Ri[k] - Rj[k];
  mv3(D, pcb, a);
  mm3(Ri, Rcb, Rb);
  mv3(Rb, dp, b);
  for (int k = 0; k < 3; k++)
    v[k] = -1.0 / dt * (s * (Twc_i[4 * k + 3] - Twc_j[4 * k + 3]) + a[k] + dt * dt / 2 * gw[k] + b[k]);
}

}  // namespace vieo
