// sim3_optimize_device.h -- the lane functions of Optimizer::OptimizeSim3 (sim3_optimize.hip; reference
// src/Optimizer.cc:2689-2918): both edge modes of EdgeReproject<2, 6, 3, MODE> (src/Odom/g2otypes.h:321-549) with their
// Jacobians as written there, Huber, the dense LDL^T, NavState::IncSmall, g2o's Levenberg-Marquardt (the policy arithmetic
// is lba_policy.h's) and the optimize(5) -> erase -> optimize(5 | 10) -> erase sequence, templated on a functor that runs
// a lane function on every lane and sums what the lanes return.  Plain functions on plain doubles: the file also compiles
// as ordinary C++, where a functor of 1 or 64 lanes runs the entire optimisation on a host (tests/emul/sim3_opt_emul.cc).
//
// The expressions of MODE 2 (EdgeReprojectPRSInv) are restated literally, not derived: scale = 1 / s, the state inverted,
// `tcw *= scale` (which scales tcb too), only the POSITION block multiplied by -Rbw, the scale column
// (J_s + Jproj tcw) (-scale^2).  tests/test_loop_optimize.py records how each block relates to central differences.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "cam_project.h"
#include "lba_policy.h"
#include "sim3_device.h"

#ifdef __HIPCC__
#define VIEO_S3O_FN __device__ __forceinline__
#define VIEO_S3O_CALL __device__ __noinline__  // the big lane functions: one body each, called
#else
#define VIEO_S3O_FN static inline
#define VIEO_S3O_CALL static inline
#endif

namespace vieo {

struct S3oCorr {         // one correspondence (112 bytes)
  double X1[3], X2[3];   // P3D1c = R1w Xw1 + t1w, P3D2c = R2w Xw2 + t2w: formed in float, widened
  double obs1[2], obs2[2];
  double info1, info2;   // (float)vinvlevelsigma2_[octave], widened
  int32_t cam1, cam2;    // the camera of e12 / e21 in the call's camera table
  int32_t i1, i2;        // the keys
};

struct S3oState {  // VertexNavStatePR + VertexScale
  double p[3];     // mpwb
  double q[4];     // mRwb, unit quaternion x, y, z, w
  double s;
};

struct S3oVisit {  // what one wavefront works on
  S3oState st;     // at entry
  double th2, delta, dsqr;  // (double)th2; Huber: (double)(float)sqrt(th2) and its square
  int32_t first, n;         // correspondences [first, first + n)
  int32_t fix_scale, pad;
};

struct S3oOut {
  S3oState st;
  int32_t n_inliers, n_bad, returned0, n_trials;
  int32_t iterations[2], trials[2];
};

enum { S3O_MAX_TRIALS = 150, S3O_ACC = 36 };  // accumulators: H upper triangle (28), b (7), robust chi2

struct S3oView {  // the arrays of one visit
  const S3oCorr* corr;
  const CamD* cams;
  int n;
  double* chi;        // [n][2] chi2_12, chi2_21 of the latest error pass (what a check reads)
  double* chi_check;  // [2][n][2] as read at the two checks
  int32_t* erased;    // [n] 0: active, 1 / 2: erased at the first / second check
  double* trace;      // [S3O_MAX_TRIALS][4] chi2 before, chi2 after, lambda, accepted
};

// ---- the state
VIEO_S3_HD void s3o_quat_normalize(double* q) {
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  q[0] /= n, q[1] /= n, q[2] /= n, q[3] /= n;
}

// ns.mRwb = SO3exd(g2oS12.rotation()).inverse(), ns.mpwb = -(ns.mRwb * g2oS12.translation()); q12 = Quaterniond(R12)
VIEO_S3_HD void s3o_state_from_sim3(const double* R12, const double* t12, double s12, S3oState& st) {
  double q[4];
  s3_mat_to_quat(R12, q);
  s3o_quat_normalize(q);
  st.q[0] = -q[0], st.q[1] = -q[1], st.q[2] = -q[2], st.q[3] = q[3];
  s3o_quat_normalize(st.q);
  double r[3];
  s3_quat_rot(st.q, t12, r);
  st.p[0] = -r[0], st.p[1] = -r[1], st.p[2] = -r[2];
  st.s = s12;
}

// R12 = ns.mRwb.inverse(); g2oS12 = Sim3(R12.unit_quaternion(), -(R12 * ns.mpwb), scale)
VIEO_S3_HD void s3o_state_to_sim3(const S3oState& st, double* R12, double* t12, double* s12) {
  double q[4] = {-st.q[0], -st.q[1], -st.q[2], st.q[3]};
  s3o_quat_normalize(q);
  double r[3];
  s3_quat_rot(q, st.p, r);
  t12[0] = -r[0], t12[1] = -r[1], t12[2] = -r[2];
  s3_quat_to_mat(q, R12);
  *s12 = st.s;
}

// NavState::IncSmall with USE_P_PLUS_RDP (NavState.h:47-58): p += Rwb * dp (the quaternion's _transformVector), Rwb *=
// Exp(dphi) (SO3ex::exp with its 1e-5 branch; both the factor and the product are normalised); VertexScale: s += ds.
VIEO_S3_HD void s3o_inc_small(S3oState& st, const double* d, bool fix_scale) {
  double r[3];
  s3_quat_rot(st.q, d, r);
  st.p[0] += r[0], st.p[1] += r[1], st.p[2] += r[2];
  const double theta = sqrt(d[3] * d[3] + d[4] * d[4] + d[5] * d[5]);
  double imag, real;
  S3_TAP(9, theta < 1e-5 ? 1.0 : 0.0) S3_TAP(10, theta)  // (sim3_device.h: empty unless a test program defines it)
  if (theta < 1e-5) {
    const double t2 = theta * theta;
    imag = 0.5 - t2 / 48.;
    real = 1.0 - t2 / 8.;
  } else {
    const double half = 0.5 * theta;
    imag = sin(half) / theta;
    real = cos(half);
  }
  double e[4] = {imag * d[3], imag * d[4], imag * d[5], real};
  s3o_quat_normalize(e);
  double o[4];
  s3_quat_mul(st.q, e, o);
  s3o_quat_normalize(o);
  st.q[0] = o[0], st.q[1] = o[1], st.q[2] = o[2], st.q[3] = o[3];
  if (!fix_scale) st.s += d[6];
}

// ---- the edges.  MODE 1: EdgeReprojectPRS (X = the candidate's point, into kf1), MODE 2: EdgeReprojectPRSInv (X = kf1's
// point, into the candidate).  Rwb = st's rotation matrix.  e[2] = obs - cam_project(Pc); J[2][7] (when J != nullptr) =
// _jacobianOplus[1] (dP, dPhi) and _jacobianOplus[2] (ds).  Every 3-term product is summed left to right.
#define S3O_DOT3(a0, a1, a2, b0, b1, b2) (((a0) * (b0) + (a1) * (b1)) + (a2) * (b2))
template <int MODE>
VIEO_S3O_CALL void s3o_edge(const CamD& c, const double* Rwb, const double* p, double s, const double* X, const double* obs,
                          double* e, double* J) {
  double scale = s;
  double Rcw[9], tcw[3], Xw[3], Pc[3];
  if (MODE == 2) {
    scale = 1. / scale;
    // Rwb' = Rwb^T, twb' = -(Rwb' * twb); Rcw = Rcb * Rwb'^T = Rcb * Rwb
    double twb[3];
    for (int i = 0; i < 3; i++) twb[i] = -S3O_DOT3(Rwb[i], Rwb[3 + i], Rwb[6 + i], p[0], p[1], p[2]);
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) Rcw[3 * i + j] = S3O_DOT3(c.Rcb[3 * i], c.Rcb[3 * i + 1], c.Rcb[3 * i + 2], Rwb[j], Rwb[3 + j], Rwb[6 + j]);
    for (int i = 0; i < 3; i++)
      tcw[i] = (-S3O_DOT3(Rcw[3 * i], Rcw[3 * i + 1], Rcw[3 * i + 2], twb[0], twb[1], twb[2]) + c.tcb[i]) * scale;
  } else {
    for (int i = 0; i < 3; i++)  // Rcw = Rcb * Rwb^T
      for (int j = 0; j < 3; j++)
        Rcw[3 * i + j] = S3O_DOT3(c.Rcb[3 * i], c.Rcb[3 * i + 1], c.Rcb[3 * i + 2], Rwb[3 * j], Rwb[3 * j + 1], Rwb[3 * j + 2]);
    for (int i = 0; i < 3; i++) tcw[i] = -S3O_DOT3(Rcw[3 * i], Rcw[3 * i + 1], Rcw[3 * i + 2], p[0], p[1], p[2]) + c.tcb[i];
  }
  for (int i = 0; i < 3; i++) Xw[i] = X[i] * scale;
  for (int i = 0; i < 3; i++) Pc[i] = S3O_DOT3(Rcw[3 * i], Rcw[3 * i + 1], Rcw[3 * i + 2], Xw[0], Xw[1], Xw[2]) + tcw[i];
  double uv[2], Jp[6];
  cam_project(c, Pc, uv, J ? Jp : nullptr);
  e[0] = obs[0] - uv[0], e[1] = obs[1] - uv[1];
  if (!J) return;
  for (int i = 0; i < 6; i++) Jp[i] = -Jp[i];  // Jproj = -d(u, v) / dPc
  for (int r = 0; r < 2; r++) {
    const double* jp = Jp + 3 * r;
    double* Jr = J + 7 * r;
    double A[3], M[3], J0[3];
    for (int j = 0; j < 3; j++) A[j] = S3O_DOT3(jp[0], jp[1], jp[2], -c.Rcb[j], -c.Rcb[3 + j], -c.Rcb[6 + j]);  // Jproj * (-Rcb)
    for (int j = 0; j < 3; j++) J0[j] = S3O_DOT3(jp[0], jp[1], jp[2], Rcw[j], Rcw[3 + j], Rcw[6 + j]);          // Jproj * Rcw
    double v[3];
    if (MODE == 2) {
      for (int j = 0; j < 3; j++) M[j] = S3O_DOT3(jp[0], jp[1], jp[2], -Rcw[j], -Rcw[3 + j], -Rcw[6 + j]);  // Jproj * (-Rcw)
      v[0] = Xw[0], v[1] = Xw[1], v[2] = Xw[2];                                                            // hat(Pw)
      for (int j = 0; j < 3; j++) Jr[j] = S3O_DOT3(A[0], A[1], A[2], -Rwb[j], -Rwb[3 + j], -Rwb[6 + j]);   // ... *= -Rbw
    } else {
      for (int j = 0; j < 3; j++) M[j] = S3O_DOT3(jp[0], jp[1], jp[2], c.Rcb[j], c.Rcb[3 + j], c.Rcb[6 + j]);  // Jproj * Rcb
      const double d0 = Xw[0] - p[0], d1 = Xw[1] - p[1], d2 = Xw[2] - p[2];  // Paux = Rwb^T (Pw - pwb)
      for (int j = 0; j < 3; j++) v[j] = S3O_DOT3(Rwb[j], Rwb[3 + j], Rwb[6 + j], d0, d1, d2);
      Jr[0] = A[0], Jr[1] = A[1], Jr[2] = A[2];
    }
    // M * hat(v)
    Jr[3] = (M[0] * 0. + M[1] * v[2]) + M[2] * -v[1];
    Jr[4] = (M[0] * -v[2] + M[1] * 0.) + M[2] * v[0];
    Jr[5] = (M[0] * v[1] + M[1] * -v[0]) + M[2] * 0.;
    double js = S3O_DOT3(J0[0], J0[1], J0[2], X[0], X[1], X[2]);  // _jacobianOplus[0] * Ph_unscale
    if (MODE == 2) js = (js + S3O_DOT3(jp[0], jp[1], jp[2], tcw[0], tcw[1], tcw[2])) * (-scale * scale);
    Jr[6] = js;
  }
}

// RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91)
VIEO_S3O_FN void s3o_huber(double e2, double delta, double dsqr, double* r0, double* r1) {
  if (e2 <= dsqr) {
    *r0 = e2, *r1 = 1.;
  } else {
    const double sq = sqrt(e2);
    *r0 = 2 * sq * delta - dsqr;
    *r1 = delta / sq;
  }
}

VIEO_S3O_FN double s3o_chi2(const double* e, double info) { return e[0] * (info * e[0]) + e[1] * (info * e[1]); }

// BaseMultiEdge::constructQuadraticForm of one edge: b += J^T (rho' Omega)(-e), H += J^T (rho' Omega) J (upper triangle,
// packed by rows, 7 columns), acc[35] += rho[0]
VIEO_S3O_FN void s3o_add_edge(const double* e, const double* J, double info, double chi2, double delta, double dsqr, double* acc) {
  double r0, r1;
  s3o_huber(chi2, delta, dsqr, &r0, &r1);
  const double w = r1 * info;
  const double o0 = -(info * e[0]) * r1, o1 = -(info * e[1]) * r1;  // omega_r = -(Omega e) rho[1]
  int k = 0;
  for (int i = 0; i < 7; i++) {
    const double a0 = J[i] * w, a1 = J[7 + i] * w;  // (J^T Omega) row i
    for (int j = i; j < 7; j++, k++) acc[k] += a0 * J[j] + a1 * J[7 + j];
    acc[28 + i] += J[i] * o0 + J[7 + i] * o1;
  }
  acc[35] += r0;
}

// One lane's share of computeActiveErrors + buildSystem: its correspondences are lane, lane + n_lanes, ...
VIEO_S3O_FN void s3o_lane_linearize(const S3oView& V, const S3oVisit& P, const S3oState& st, int lane, int n_lanes, double* acc) {
  for (int i = 0; i < S3O_ACC; i++) acc[i] = 0;
  double Rwb[9];
  s3_quat_to_mat(st.q, Rwb);
  for (int k = lane; k < V.n; k += n_lanes) {
    if (V.erased[k]) continue;
    const S3oCorr& C = V.corr[k];
    double e[2], J[14];
    s3o_edge<1>(V.cams[C.cam1], Rwb, st.p, st.s, C.X2, C.obs1, e, J);
    const double c12 = s3o_chi2(e, C.info1);
    s3o_add_edge(e, J, C.info1, c12, P.delta, P.dsqr, acc);
    s3o_edge<2>(V.cams[C.cam2], Rwb, st.p, st.s, C.X1, C.obs2, e, J);
    const double c21 = s3o_chi2(e, C.info2);
    s3o_add_edge(e, J, C.info2, c21, P.delta, P.dsqr, acc);
    V.chi[2 * k] = c12, V.chi[2 * k + 1] = c21;
  }
}

// computeActiveErrors + activeRobustChi2
VIEO_S3O_FN double s3o_lane_errors(const S3oView& V, const S3oVisit& P, const S3oState& st, int lane, int n_lanes) {
  double sum = 0;
  double Rwb[9];
  s3_quat_to_mat(st.q, Rwb);
  for (int k = lane; k < V.n; k += n_lanes) {
    if (V.erased[k]) continue;
    const S3oCorr& C = V.corr[k];
    double e[2], r0, r1;
    s3o_edge<1>(V.cams[C.cam1], Rwb, st.p, st.s, C.X2, C.obs1, e, nullptr);
    const double c12 = s3o_chi2(e, C.info1);
    s3o_huber(c12, P.delta, P.dsqr, &r0, &r1);
    sum += r0;
    s3o_edge<2>(V.cams[C.cam2], Rwb, st.p, st.s, C.X1, C.obs2, e, nullptr);
    const double c21 = s3o_chi2(e, C.info2);
    s3o_huber(c21, P.delta, P.dsqr, &r0, &r1);
    sum += r0;
    V.chi[2 * k] = c12, V.chi[2 * k + 1] = c21;
  }
  return sum;
}

// a check (Optimizer.cc:2858-2874, :2891-2905): reads the errors the edges hold; returns how many it erased
VIEO_S3O_FN double s3o_lane_check(const S3oView& V, const S3oVisit& P, int check, int lane, int n_lanes) {
  double erased = 0;
  for (int k = lane; k < V.n; k += n_lanes) {
    if (V.erased[k]) continue;
    const double c12 = V.chi[2 * k], c21 = V.chi[2 * k + 1];
    V.chi_check[((size_t)check * V.n + k) * 2] = c12, V.chi_check[((size_t)check * V.n + k) * 2 + 1] = c21;
    if (c12 > P.th2 || c21 > P.th2) V.erased[k] = check + 1, erased += 1;
  }
  return erased;
}

// (H + lambda I) x = b by LDL^T without pivoting on the leading N x N block of the packed upper triangle; false on a
// non-positive pivot (g2o: the trial fails, lambda grows).  Runs uniformly on every lane.
template <int N>
VIEO_S3O_FN bool s3o_ldlt_solve(const double* acc, double lambda, double* x) {
  double L[N][N], D[N];
  int k = 0;
  for (int i = 0; i < 7; i++)
    for (int j = i; j < 7; j++, k++)
      if (j < N) L[j][i] = acc[k];  // lower triangle <- the upper one
  for (int j = 0; j < N; j++) {
    double d = L[j][j] + lambda;
    for (int q = 0; q < j; q++) d -= L[j][q] * L[j][q] * D[q];
    if (!(d > 0)) return false;
    D[j] = d;
    for (int i = j + 1; i < N; i++) {
      double a = L[i][j];
      for (int q = 0; q < j; q++) a -= L[i][q] * L[j][q] * D[q];
      L[i][j] = a / d;
    }
  }
  double y[N];
  for (int i = 0; i < N; i++) {
    double a = acc[28 + i];
    for (int q = 0; q < i; q++) a -= L[i][q] * y[q];
    y[i] = a;
  }
  for (int i = N - 1; i >= 0; i--) {
    double a = y[i] / D[i];
    for (int q = i + 1; q < N; q++) a -= L[q][i] * x[q];
    x[i] = a;
  }
  return true;
}

// SparseOptimizer::optimize(iters) with OptimizationAlgorithmLevenberg::solve (optimization_algorithm_levenberg.cpp:61-189).
// Lanes::run<N>(f, out): f(lane, n_lanes, part) on every lane, out[0..N) = the sums of part[0..N) over the lanes, the same
// on every lane; Lanes::leader(): the one lane that writes the trace.  The errors in V.chi after the call are those of the
// LAST lambda trial, accepted or not: pop() does not restore them.  dim = 6 (fixed scale) or 7.
template <class Lanes>
VIEO_S3O_FN void s3o_optimize(Lanes& L, const S3oView& V, const S3oVisit& P, S3oState& st, int dim, int iters, int32_t* n_trace,
                              int32_t* iterations, int32_t* trials) {
  LmCore c;
  double acc[S3O_ACC], x[7];
  *iterations = 0, *trials = 0;
  if (iters <= 0) return;
  for (;;) {
    L.template run<S3O_ACC>([&](int lane, int nl, double* part) { s3o_lane_linearize(V, P, st, lane, nl, part); }, acc);
    ++*iterations;
    c.currentChi = acc[35], c.iniChi = acc[35];
    if (c.it == 0) {  // computeLambdaInit: tau * the largest diagonal entry
      double m = 0;
      int k = 0;
      for (int i = 0; i < 7; i++) {
        if (i < dim) m = fabs(acc[k]) > m ? fabs(acc[k]) : m;
        k += 7 - i;
      }
      c.lambda = 1e-5 * m, c.ni = 2, c.nBad = 0;
    }
    c.qmax = 0;
    double rho;
    do {
      const S3oState backup = st;  // push()
      for (int i = 0; i < 7; i++) x[i] = 0;
      const bool ok2 = dim == 6 ? s3o_ldlt_solve<6>(acc, c.lambda, x) : s3o_ldlt_solve<7>(acc, c.lambda, x);
      if (!ok2)
        for (int i = 0; i < 7; i++) x[i] = 0;
      s3o_inc_small(st, x, dim == 6);
      double chi;
      L.template run<1>([&](int lane, int nl, double* part) { part[0] = s3o_lane_errors(V, P, st, lane, nl); }, &chi);
      double scale = 0;  // computeScale (x[6] = 0 when the scale is fixed)
      for (int j = 0; j < 7; j++) scale += x[j] * (c.lambda * x[j] + acc[28 + j]);
      const double before = c.currentChi, lambda = c.lambda;
      bool accepted;
      rho = lm_core_trial(c, ok2, chi, scale, &accepted);
      if (!accepted) st = backup;  // pop()
      if (L.leader() && *n_trace < S3O_MAX_TRIALS) {
        double* t = V.trace + 4 * *n_trace;
        t[0] = before, t[1] = ok2 ? chi : DBL_MAX, t[2] = lambda, t[3] = accepted ? 1. : 0.;
      }
      ++*n_trace, ++*trials;
    } while (rho < 0 && c.qmax < 10);
    if (lm_core_iteration_end(c, rho, iters, false)) return;
  }
}

// Optimizer::OptimizeSim3 after the edges are set: optimize(5), the first check, optimize(nMore), the second check
template <class Lanes>
VIEO_S3O_FN void s3o_visit(Lanes& L, const S3oView& V, const S3oVisit& P, S3oOut& O) {
  S3oState st = P.st;
  O.n_trials = 0, O.returned0 = 0, O.n_inliers = 0, O.n_bad = 0;
  O.iterations[1] = 0, O.trials[1] = 0;
  O.st = P.st;
  int iters = 5;
  for (int stage = 0; stage < 2; stage++) {
    s3o_optimize(L, V, P, st, P.fix_scale ? 6 : 7, iters, &O.n_trials, &O.iterations[stage], &O.trials[stage]);
    double cnt;
    L.template run<1>([&](int lane, int nl, double* part) { part[0] = s3o_lane_check(V, P, stage, lane, nl); }, &cnt);
    if (stage == 0) {
      O.n_bad = (int)cnt;
      iters = O.n_bad > 0 ? 10 : 5;
      if (V.n - O.n_bad < 10) {  // `return 0` before g2oS12 is written back
        O.returned0 = 1;
        return;
      }
    } else
      O.n_inliers = V.n - O.n_bad - (int)cnt;
  }
  O.st = st;
}

}  // namespace vieo
