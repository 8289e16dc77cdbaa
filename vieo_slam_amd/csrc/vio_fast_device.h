// vio_fast_device.h -- the fast single-lane forms of k_pose_opt_vio (pose_opt_vio.hip): polynomial Exp / Log / Jr / JrInv,
// the prior and inertial edges that hand a RotCache from the error evaluation to the linearisation, the straight-line
// visual edge and the one-wavefront LDL^T solver.  A header so that tests/hip_unit/vio_fast_test.hip can call them lane by
// lane.  The including translation unit sets `#pragma clang fp contract(fast)` BEFORE this header: the forms are meant to
// be compiled with fused multiply-adds (see pose_opt_vio.hip).
#pragma once
#include "imu_device.h"

namespace vieo {

// ---- the single-lane edges, round 6: what an error evaluation has computed is not computed again by the linearisation
// that follows it at the same state (the LM loop linearises at the state of the last accepted -- i.e. last -- evaluation).
// A lane's time here is the latency of its transcendental chains (sincos 374 cycles, atan 211, sqrt 101, a division 76,
// tools/micro/lat_bench.hip), so the rules are: (1) a quaternion that is a product of unit quaternions is re-normalised
// by the series of 1 / sqrt(1 + e) (|e| ~ 1e-16: exact to rounding) instead of sqrt + division; (2) Exp(-Log(q)) is
// conj(q); (3) JrInv(Log(q)) and Jr(w) take sin / cos of the angle from the half-angle values the quaternion / the
// exponential already hold (sin t = 2 s c, 1 + cos t = 2 c^2, 1 - cos t = 2 s^2); (4) constants of the call (the
// quaternion of the pre-integrated rotation) are formed once.  Values agree with the plain forms (imu_device.h, kept
// for the local BA) to rounding; the optimiser's parity bar is 1e-4 on SE(3).
// (5) Inside |angle| < ~0.5 rad -- every increment, bias correction and edge error of a tracked frame -- Exp, Log, Jr and
// JrInv are polynomials in the squared angle (Taylor series to double rounding: the remainders are below 1e-17 on the
// stated domains): no sqrt, no sincos, no atan, one or two reciprocals.  Outside the domain the plain forms run.
//   cos(t/2) = sum (-1)^k u^k / (4^k (2k)!),  sin(t/2) / t = sum (-1)^k u^k / (2 4^k (2k+1)!),  u = t^2 < 1/4
//   Jr(w) = I - A hat(w) + B hat(w)^2,  A = (1 - cos t) / t^2 = sum (-1)^k u^k / (2k+2)!,  B = (t - sin t) / t^3 = sum (-1)^k u^k / (2k+3)!
//   Log(w, v) = (2 P / w) v with x^2 = |v|^2 / w^2 < 1/16, P = atan(x) / x = 1 - x^2 Q, Q = 1/3 - x^2/5 + x^4/7 - ...
//   JrInv(Log q) = I + hat(e) / 2 + g hat(e)^2,  g = (1 - t (1 + cos t) / (2 sin t)) / t^2 = Q / (4 P^2)   (-> 1/12 at 0)
constexpr double kCosH[9] = {1.0, -0.125, 0.0026041666666666665, -2.170138888888889e-05, 9.68812003968254e-08, -2.691144455467372e-10, 5.096864498991235e-13, -7.001187498614334e-16, 7.292903644389931e-19};
constexpr double kSinHT[9] = {0.5, -0.020833333333333332, 0.00026041666666666666, -1.5500992063492063e-06, 5.382288910934745e-09, -1.2232474797578965e-11, 1.9603324996120133e-14, -2.333729166204778e-17, 2.1449716601146855e-20};
constexpr double kJrA[9] = {0.5, -0.041666666666666664, 0.001388888888888889, -2.48015873015873e-05, 2.755731922398589e-07, -2.08767569878681e-09, 1.1470745597729725e-11, -4.779477332387385e-14, 1.5619206968586225e-16};
constexpr double kJrB[9] = {0.16666666666666666, -0.008333333333333333, 0.0001984126984126984, -2.7557319223985893e-06, 2.505210838544172e-08, -1.6059043836821613e-10, 7.647163731819816e-13, -2.8114572543455206e-15, 8.22063524662433e-18};
constexpr double kAtanQ[16] = {0.3333333333333333, -0.2, 0.14285714285714285, -0.1111111111111111, 0.09090909090909091, -0.07692307692307693, 0.06666666666666667, -0.058823529411764705, 0.05263157894736842, -0.047619047619047616, 0.043478260869565216, -0.04, 0.037037037037037035, -0.034482758620689655, 0.03225806451612903, -0.030303030303030304};
// (6) The hot forms are STRAIGHT-LINE code: a lane's error evaluation is one basic block in which the scheduler
// interleaves the independent chains (position / velocity rows beside the quaternion chain of the rotation rows) --
// with a branch per domain test each piece was a block of its own and the lane ran them one dependent instruction at a
// time.  Every polynomial is evaluated unconditionally, the domain tests only clear `ok`, and a caller whose evaluation
// ends with ok == false (angles beyond the domains, a quaternion that is not unit: never in a tracked sequence) runs
// the plain forms of imu_device.h after it.
__device__ __forceinline__ Qd q_renorm(const Qd& q, bool& ok) {
  const double e = (q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z) - 1.0;
  ok = ok && fabs(e) < 1e-5;
  const double r = 1.0 - e * (0.5 - 0.375 * e);
  return Qd{q.w * r, q.x * r, q.y * r, q.z * r};
}
template <int N>
__device__ __forceinline__ double horner(const double (&c)[N], double u) {
  double r = c[N - 1];
#pragma unroll
  for (int k = N - 2; k >= 0; k--) r = __builtin_fma(r, u, c[k]);
  return r;
}
__device__ __forceinline__ double rcp_nr(double d) {  // 1 / d: v_rcp_f64 + two Newton steps (as the solver's pivots)
  double inv = __builtin_amdgcn_rcp(d);
  inv = __builtin_fma(__builtin_fma(-d, inv, 1.0), inv, inv);
  return __builtin_fma(__builtin_fma(-d, inv, 1.0), inv, inv);
}
// SO3ex::exp (so3_extra.h:121-142) as a unit quaternion; domain |w|^2 < 1/4
__device__ __forceinline__ Qd so3_exp_unit(const double* w, bool& ok) {
  const double u = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  ok = ok && u < 0.25;
  const double real = horner(kCosH, u), imag = horner(kSinHT, u);
  return q_renorm(Qd{real, imag * w[0], imag * w[1], imag * w[2]}, ok);
}
// SO3ex::log (so3_extra.h:144-190) of a unit quaternion, and g of JacobianRInv(log) = I + hat / 2 + g hat^2;
// domain tan^2(half angle) < 1/16
__device__ __forceinline__ void so3_log_unit(const Qd& q, double* out, double* g, bool& ok) {
  const double n2 = q.x * q.x + q.y * q.y + q.z * q.z, w2 = q.w * q.w;
  ok = ok && n2 < 0.0625 * w2;
  const double iw = rcp_nr(q.w), x2 = n2 * (iw * iw);
  const double Q = horner(kAtanQ, x2), P = __builtin_fma(-x2, Q, 1.0);
  const double f = 2.0 * P * iw;
  out[0] = f * q.x, out[1] = f * q.y, out[2] = f * q.z;
  *g = Q * rcp_nr(4.0 * P * P);
}
// g of JacobianRInv for an angle outside the polynomial's domain (the plain forms' fallback)
__device__ __forceinline__ double so3_JrInv_g_of_inl(const double* e) {
  const double th2 = e[0] * e[0] + e[1] * e[1] + e[2] * e[2], th = sqrt(th2);
  if (th < 1e-5) return 1. / 12.;
  double sth, cth;
  sincos(th, &sth, &cth);
  return (1.0 - (1.0 + cth) * th / (2.0 * sth)) / th2;
}
__device__ __noinline__ double so3_JrInv_g_of(const double* e) { return so3_JrInv_g_of_inl(e); }
__device__ __forceinline__ void so3_JrInv_g(const double* e, double g, double* J) {
  // hat(e)^2 = e e^T - |e|^2 I
  const double xx = e[0] * e[0], yy = e[1] * e[1], zz = e[2] * e[2];
  const double xy = g * e[0] * e[1], xz = g * e[0] * e[2], yz = g * e[1] * e[2];
  J[0] = 1.0 - g * (yy + zz), J[1] = xy - 0.5 * e[2], J[2] = xz + 0.5 * e[1];
  J[3] = xy + 0.5 * e[2], J[4] = 1.0 - g * (xx + zz), J[5] = yz - 0.5 * e[0];
  J[6] = xz - 0.5 * e[1], J[7] = yz + 0.5 * e[0], J[8] = 1.0 - g * (xx + yy);
}
// JacobianR(w) (so3_extra.h:254-270); domain |w|^2 < 1/4 (the caller knows from the cache)
__device__ __forceinline__ void so3_Jr_unit(const double* w, double* J) {
  const double u = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  const double A = horner(kJrA, u), B = horner(kJrB, u);
  const double xx = w[0] * w[0], yy = w[1] * w[1], zz = w[2] * w[2];
  const double xy = B * w[0] * w[1], xz = B * w[0] * w[2], yz = B * w[1] * w[2];
  J[0] = 1.0 - B * (yy + zz), J[1] = xy + A * w[2], J[2] = xz - A * w[1];
  J[3] = xy - A * w[2], J[4] = 1.0 - B * (xx + zz), J[5] = yz + A * w[0];
  J[6] = xz + A * w[1], J[7] = yz - A * w[0], J[8] = 1.0 - B * (xx + yy);
}
struct RotCache {  // written by an error evaluation, read by the linearisation at the same state
  Qd qe, qb;        // inertial edge: the error quaternion (err_R = Log qe) and conj(q_i) q_j
  double g_e;       // JrInv(err_R) = I + hat / 2 + g_e hat^2
  double w[3];      // JgR dbg_i
  Qd qp;            // prior edge: conj(q_prior) q_i, err_P[6..9) = Log qp
  double g_p;
  int w_small;      // |w|^2 < 1/4: Jr(w) by its polynomial
};

// EdgeNavStatePriorPVRBias (g2otypes.cpp:84-124); J is 15 x 15: cols 0..8 PVR_i, 9..14 Bias_i
// LEAF: the fallback is inlined (the callers that are out-of-line functions themselves: a call inside them would make
// them save a register to scratch memory on every entry)
template <bool LEAF = false>
__device__ __forceinline__ void prior_error(const NSd& pr, const NSd& si, double* err, RotCache& C) {
  double Rb[9], d[3];
  q_to_R(q_of(pr), Rb);
  for (int k = 0; k < 3; k++) d[k] = si.p[k] - pr.p[k];
  mTv3(Rb, d, err);
  bool ok = true;
  Qd q = q_renorm(q_mul(q_conj(q_of(pr)), q_of(si)), ok);
  double g;
  so3_log_unit(q, err + 6, &g, ok);
  for (int k = 0; k < 3; k++) {
    err[3 + k] = si.v[k] - pr.v[k];
    err[9 + k] = si.bg[k] + si.dbg[k] - (pr.bg[k] + pr.dbg[k]);
    err[12 + k] = si.ba[k] + si.dba[k] - (pr.ba[k] + pr.dba[k]);
  }
  if (!ok) {  // the plain forms
    q = q_norm(q_mul(q_conj(q_of(pr)), q_of(si)));
    so3_log_q(q, err + 6);
    g = LEAF ? so3_JrInv_g_of_inl(err + 6) : so3_JrInv_g_of(err + 6);
  }
  C.qp = q, C.g_p = g;
}
// The Jacobian's constant part (zeros, the three identity blocks) is written once per call (prior_jacobian_init, all
// threads); a linearisation writes the two blocks that depend on the state: R_prior^T R_i = R(conj(q_prior) q_i), the
// quaternion the error evaluation formed, and JrInv of the rotation error.
__device__ __forceinline__ void prior_jacobian_init(double* J, int tid, int nthreads) {
  for (int e = tid; e < 225; e += nthreads) {
    const int r = e / 15, c = e - r * 15;
    J[e] = (r == c && ((r >= 3 && r < 6) || r >= 9)) ? 1.0 : 0.0;
  }
}
__device__ __forceinline__ void prior_linearize(const double* err, double* J, const RotCache& C) {
  double tmp[9], Jrinv[9];
  q_to_R(C.qp, tmp);
  set3(J, 15, 0, 0, tmp, 1.0);
  so3_JrInv_g(err + 6, C.g_p, Jrinv);
  set3(J, 15, 6, 6, Jrinv, 1.0);
}

// EdgeNavStateI computeError, rotation rows (imu_device.h imu_error part 2) with the intermediates kept; qRij = the
// quaternion of the pre-integrated rotation (R_to_q(M.Rij), once per call)
template <bool LEAF = false>
__device__ __forceinline__ void imu_error_rot(const vieo_imu_preint& M, const Qd& qRij, const NSd& si, const NSd& sj, double* err, RotCache& C) {
  double w[3];
  mv3(M.JgR, si.dbg, w);
  bool ok = true;
  const Qd qx = so3_exp_unit(w, ok);
  const bool w_small = ok;
  Qd qb = q_renorm(q_mul(q_conj(q_of(si)), q_of(sj)), ok);  // (independent of the chain through qx)
  const Qd qa = q_renorm(q_mul(qRij, qx), ok);
  Qd qe = q_renorm(q_mul(q_conj(qa), qb), ok);
  double g;
  so3_log_unit(qe, err + 6, &g, ok);
  if (!ok) {  // the plain forms
    qb = q_norm(q_mul(q_conj(q_of(si)), q_of(sj)));
    qe = q_norm(q_mul(q_conj(q_norm(q_mul(qRij, so3_exp_q(w)))), qb));
    so3_log_q(qe, err + 6);
    g = LEAF ? so3_JrInv_g_of_inl(err + 6) : so3_JrInv_g_of(err + 6);
  }
  C.qe = qe, C.qb = qb, C.g_e = g;
  C.w[0] = w[0], C.w[1] = w[1], C.w[2] = w[2], C.w_small = w_small ? 1 : 0;
}
// The inertial Jacobian (9 x 24, imu_device.h imu_linearize with (idR, idV) = (6, 3)) has 14 non-zero 3 x 3 blocks, five
// of them constants of the call (-I and the four bias Jacobians of the pre-integration): those and the zeros are
// written once (imu_jacobian_init, all threads); a linearisation writes the nine blocks that depend on the states.
__device__ __forceinline__ void imu_jacobian_init(const vieo_imu_preint& M, double* J, int tid, int nthreads) {
  for (int e = tid; e < 9 * 24; e += nthreads) {
    const int r = e / 24, c = e - r * 24;
    double v = 0.0;
    if (r < 3) {
      if (c >= 9 && c < 12) v = (c - 9 == r) ? -1.0 : 0.0;
      if (c >= 18 && c < 21) v = -M.Jgp[r * 3 + c - 18];
      if (c >= 21) v = -M.Jap[r * 3 + c - 21];
    } else if (r < 6) {
      if (c >= 18 && c < 21) v = -M.Jgv[(r - 3) * 3 + c - 18];
      if (c >= 21) v = -M.Jav[(r - 3) * 3 + c - 21];
    }
    J[e] = v;
  }
}
// position and velocity rows (imu_linearize part 1 without its constant blocks)
__device__ __forceinline__ void imu_linearize_pv(const vieo_imu_preint& M, const double* gw, const NSd& si, const NSd& sj, double* J) {
  const int ld = 24, cj = 0, ci = 9, idR = 6, idV = 3;
  double Ri[9], RiT[9], Rj[9], t[3], r[3], Hm[9], tmp[9];
  q_to_R(q_of(si), Ri);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) RiT[i * 3 + j] = Ri[j * 3 + i];
  q_to_R(q_of(sj), Rj);
  const double dt = M.dt;
  for (int k = 0; k < 3; k++) t[k] = sj.p[k] - si.p[k] - si.v[k] * dt - gw[k] * (dt * dt / 2);
  mv3(RiT, t, r);
  hat3(r, Hm);
  set3(J, ld, 0, ci + idR, Hm, 1.0);
  set3(J, ld, 0, ci + idV, RiT, -dt);
  mm3(RiT, Rj, tmp);
  set3(J, ld, 0, cj + 0, tmp, 1.0);
  for (int k = 0; k < 3; k++) t[k] = sj.v[k] - si.v[k] - gw[k] * dt;
  mv3(RiT, t, r);
  hat3(r, Hm);
  set3(J, ld, idV, ci + idR, Hm, 1.0);
  set3(J, ld, idV, ci + idV, RiT, -1.0);
  set3(J, ld, idV, cj + idV, RiT, 1.0);
}
// EdgeNavStateI linearizeOplus, rotation rows (imu_device.h imu_linearize part 2; the caller has cleared J) from the
// cache of the error evaluation at the same state
__device__ __forceinline__ void imu_linearize_rot(const vieo_imu_preint& M, const double* err, double* J, const RotCache& C) {
  const int ld = 24, cj = 0, ci = 9, cb = 18, idR = 6;
  double Jrinv[9], Rji[9], tmp[9], tmp2[9], E[9], Jr[9];
  so3_JrInv_g(err + idR, C.g_e, Jrinv);
  q_to_R(q_conj(C.qb), Rji);                    // R_j^T R_i
  mm3(Jrinv, Rji, tmp);
  set3(J, ld, idR, ci + idR, tmp, -1.0);
  q_to_R(q_conj(C.qe), E);                      // Exp(-err_R)
  so3_Jr_unit(C.w, Jr);
  if (!C.w_small) so3_Jr_d(C.w, Jr);
  mm3(Jrinv, E, tmp);
  mm3(tmp, Jr, tmp2);
  mm3(tmp2, M.JgR, tmp);
  set3(J, ld, idR, cb + 0, tmp, -1.0);
  set3(J, ld, idR, cj + idR, Jrinv, 1.0);
}
// NavState::IncSmall(dPVR) + IncSmallBias (imu_device.h ns_inc)
__device__ __forceinline__ void ns_inc_unit(NSd& s, const double* d, const double* db) {
  double R[9], Rd[3];
  q_to_R(q_of(s), R);
  mv3(R, d, Rd);
  bool ok = true;
  Qd q = q_renorm(q_mul(q_of(s), so3_exp_unit(d + 6, ok)), ok);
  if (!ok) q = q_norm(q_mul(q_of(s), so3_exp_q(d + 6)));
  for (int i = 0; i < 3; i++) s.p[i] += Rd[i], s.v[i] += d[3 + i];
  s.qw = q.w, s.qx = q.x, s.qy = q.y, s.qz = q.z;
  for (int i = 0; i < 3; i++) s.dbg[i] += db[i], s.dba[i] += db[3 + i];
}

// ---- the visual edges of a one-camera frame as STRAIGHT-LINE code (round 6).  A pass over the edges was a loop with a
// `continue` for the edges of the wrong level, a branch for the stereo row and one inside the Huber kernel: every edge a
// chain of basic blocks in which one wavefront per SIMD runs its ~320 double-precision instructions one dependent link
// after the other (~9 cycles each against 4 of issue).  Here an edge is evaluated unconditionally -- a masked or
// out-of-range slot with weight 0, the stereo row of a monocular edge as zeros, the Huber kernel by selection -- so that
// TWO edges form one block and the scheduler interleaves their chains.  A valid edge goes through the operations of
// edge_error / visual_jacobian / visual_accumulate (ba_device.h) in their order; the zeros added for the other slots do
// not change a sum.
struct VisFlat {
  double err[3], Pc[3], info, chi2;
  bool stereo;
};
__device__ __forceinline__ void vis_error_flat(const CamD& c, const PoseXf& X, const vieo_pose_obs& o, bool valid, VisFlat& E) {
  const double Xw0 = o.Xw[0], Xw1 = o.Xw[1], Xw2 = o.Xw[2];
  for (int i = 0; i < 3; i++) E.Pc[i] = X.Rcw[i * 3] * Xw0 + X.Rcw[i * 3 + 1] * Xw1 + X.Rcw[i * 3 + 2] * Xw2 + X.tcw[i];
  if (!valid) E.Pc[2] = 1.0;  // (a slot that does not count must not divide by a zero depth: inf x weight 0 = NaN)
  const double invz = 1. / E.Pc[2];
  const double u = (double)(float)(c.fx * E.Pc[0] * invz + c.cx);
  const double v = (double)(float)(c.fy * E.Pc[1] * invz + c.cy);
  E.err[0] = (double)o.u - u;
  E.err[1] = (double)o.v - v;
  E.info = (double)o.inv_sigma2;
  E.stereo = o.ur >= 0;
  const double e2 = (double)o.ur - (u - c.bf / E.Pc[2]);
  E.err[2] = E.stereo ? e2 : 0.0;
  const double chi = E.err[0] * (E.info * E.err[0]) + E.err[1] * (E.info * E.err[1]);
  const double chis = chi + E.err[2] * (E.info * E.err[2]);
  E.chi2 = E.stereo ? chis : chi;
}
// RobustKernelHuber::robustify by selection (huber() of ba_device.h: same values)
__device__ __forceinline__ void huber_flat(double e, double delta, double dsqr, bool robust, double* r0, double* r1) {
  const bool big = robust && !(e <= dsqr);
  const double sq = sqrt(big ? e : dsqr);
  *r0 = big ? 2 * sq * delta - dsqr : e;
  *r1 = big ? delta / sq : 1.;
}
// visual_jacobian with the stereo row of a monocular edge as zeros
__device__ __forceinline__ void vis_jacobian_flat(const CamD& c, const PoseXf& X, const double* p, const vieo_pose_obs& o,
                                                  const VisFlat& E, double* J) {
  const double invz = 1 / E.Pc[2], invz2 = invz * invz;
  double Jp[9];
  Jp[0] = -(c.fx * invz), Jp[1] = 0, Jp[2] = -(-c.fx * E.Pc[0] * invz2);
  Jp[3] = 0, Jp[4] = -(c.fy * invz), Jp[5] = -(-c.fy * E.Pc[1] * invz2);
  Jp[6] = E.stereo ? Jp[0] : 0.0, Jp[7] = 0, Jp[8] = E.stereo ? Jp[2] - c.bf * invz2 : 0.0;
  const double dP0 = (double)o.Xw[0] - p[0], dP1 = (double)o.Xw[1] - p[1], dP2 = (double)o.Xw[2] - p[2];
  double Pa[3];
  for (int m = 0; m < 3; m++) Pa[m] = X.Rwb[m] * dP0 + X.Rwb[3 + m] * dP1 + X.Rwb[6 + m] * dP2;
  double RH[9];  // Rcb * hat(Rwb^T (Xw - pwb))
  for (int m = 0; m < 3; m++) {
    const double a = c.Rcb[m * 3], b = c.Rcb[m * 3 + 1], d = c.Rcb[m * 3 + 2];
    RH[m * 3 + 0] = b * Pa[2] - d * Pa[1];
    RH[m * 3 + 1] = -a * Pa[2] + d * Pa[0];
    RH[m * 3 + 2] = a * Pa[1] - b * Pa[0];
  }
  for (int r = 0; r < 3; r++)
    for (int q = 0; q < 3; q++) {
      J[r * 6 + q] = -(Jp[r * 3] * c.Rcb[q] + Jp[r * 3 + 1] * c.Rcb[3 + q] + Jp[r * 3 + 2] * c.Rcb[6 + q]);
      J[r * 6 + 3 + q] = Jp[r * 3] * RH[q] + Jp[r * 3 + 1] * RH[3 + q] + Jp[r * 3 + 2] * RH[6 + q];
    }
}
// visual_accumulate with all three rows (the third is zero for a monocular edge) and the weight of the slot
__device__ __forceinline__ void vis_accumulate_flat(const double* J, const double* err, double info, double r1, double* acc) {
  const double w = r1 * info;
  int t = 0;
  for (int a = 0; a < 6; a++) {
    for (int b = a; b < 6; b++, t++) {
      double s = J[a] * w * J[b] + J[6 + a] * w * J[6 + b];
      s += J[12 + a] * w * J[12 + b];
      acc[t] += s;
    }
    double s = J[a] * (-(info * err[0]) * r1) + J[6 + a] * (-(info * err[1]) * r1);
    s += J[12 + a] * (-(info * err[2]) * r1);
    acc[21 + a] += s;
  }
}

// LDS hand-over between the lanes of one wavefront
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// A right-looking LDL^T with the matrix in registers: lane i owns row i of (H + lambda I), column
// values travel by v_readlane (the column index is a compile-time constant after unrolling), so the
// N pivot steps need no LDS round trip and no barrier.  The operations and their order are those of the plain
// right-looking form: l = c / d, then a_ik -= l_i * c_k.
__device__ __forceinline__ double readlane_d(double v, int srclane) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)b, srclane);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), srclane);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// The system's structure (round 4): the bias of the current state (unknowns 9..14) meets the rest of the system only
// through the random-walk edge, one diagonal entry w_t per component and -w_t towards the last state's bias (24 + t) when
// that is free -- the inertial edge's Jacobian has no column for it, the visual, prior and encoder edges neither.  Its six
// unknowns are eliminated in closed form (pivot d_t = w_t + lambda) and the factorisation runs on the remaining NR = 24
// (last state free) or 9 (last state fixed) unknowns: 0.65x / 0.25x of the dependent pivot chain of the 30 / 15-dim form.
// Reduced index r -> system index: r < 9 ? r : r + 6.  Lane r owns row r and keeps 1 / d_r; the columns broadcast during
// the factorisation stay in LDS (Ls, NR x 34 doubles) and serve the back substitution.
// (the "TP:" comments mark the phases tools/micro/gen_solve_bench.py puts its s_memtime probes at)
// The function is out of line (two instances, one call site each); its arrays are named in the LDS address space so that
// every access is a plain ds_ instruction -- through generic pointers each one carried a 64-bit address add and a null
// test of the flat -> LDS cast (3 extra instructions per access, about a third of the function).
typedef __attribute__((address_space(3))) double lds_f64;
template <int NR>
__device__ bool wave_solve_vio(const lds_f64* H, int n, double lambda, const lds_f64* b, lds_f64* x, lds_f64* Ls, int lane) {
  // the lane masks below are formed here, per call: hoisted out of the caller's trial loop they would live in ~100
  // scalar registers, i.e. be spilled to lanes of a VGPR and read back by v_readlane, two instructions per use
  asm volatile("" : "+v"(lane));
  double a[NR];
  // lanes 32..63 mirror lanes 0..31 (same row, same values, same LDS addresses): no execution mask anywhere
  const int l32 = lane & 31;
  const int row = l32 < NR ? l32 : 0;
  const int frow = row < 9 ? row : row + 6;
#pragma unroll
  for (int k = 0; k < NR; k++) a[k] = H[frow * n + (k < 9 ? k : k + 6)];  // lambda joins the pivots as they are read
  double y = l32 < NR ? b[frow] : 0.0;
  bool ok = true;
  // the six eliminated unknowns: lane t < 6 keeps its pivot's reciprocal, lanes 18 + t of the 24-dim form take the update
  double dbias = 1.0, off = 0.0;
  {
    const int t = NR == 24 ? (l32 >= 18 && l32 < 24 ? l32 - 18 : (l32 < 6 ? l32 : 0)) : (l32 < 6 ? l32 : 0);
    const double d = H[(9 + t) * n + 9 + t] + lambda;
    if (!(d > 0)) ok = false;
    double inv = __builtin_amdgcn_rcp(d);
    inv = __builtin_fma(__builtin_fma(-d, inv, 1.0), inv, inv);
    inv = __builtin_fma(__builtin_fma(-d, inv, 1.0), inv, inv);
    dbias = inv;
    if (NR == 24) {
      off = H[(9 + t) * n + 24 + t];
      const double l = l32 >= 18 && l32 < 24 ? off * inv : 0.0;
#pragma unroll
      for (int k = 18; k < 24; k++) a[k] = __builtin_fma(k == l32 ? -l : 0.0, off, a[k]);
      y = __builtin_fma(-l, b[9 + t], y);
    }
  }
  ok = __all(ok);
  // TP:factor
  // Column j travels to the other rows through LDS (one ds_write per lane, then wave-uniform -- broadcast -- reads, two
  // values per instruction) instead of two v_readlane per value: a wavefront issues one instruction every 4 cycles
  // (double precision included: tools/micro/lat_bench.hip) whatever the number of useful lanes, so the count of
  // instructions is the cost, and this form has a quarter of them.  Every column keeps its own 34 doubles of Ls, zero at and above the diagonal: together they are
  // L^T un-normalised, which is what the backward substitution reads (lane i its own column i) -- L is never stored.
  lds_f64* colbuf = Ls;  // NR x kCS doubles: 34 keeps pairs 16-byte aligned and spreads the backward pass's per-lane
  constexpr int kCS = 34;  // column reads over the banks (32 would put every lane on one bank: 32 passes per read)
  // The pivot chain -- d_j -> 1 / d_j (v_rcp_f64 + two Newton steps) -> l -> d_(j+1) -- never waits for LDS: row j + 1's
  // own update of its diagonal needs only its own two values (A[j+1][j] is its own column entry), so the next pivot is
  // formed from registers and read by v_readlane while the broadcast of column j is still on its way.
  // The forward substitution y = L^-1 b rides along (b is one more column of the row: y_j is final once pivot j starts).
  // The broadcast of column j is consumed one pivot late (cp / lp): its ds_reads are issued at the end of pivot j and
  // their values first needed after pivot j + 1's reciprocal chain, which covers the LDS round trip (~77 cycles); the
  // empty asm ties that first use to the chain's result so that the scheduler does not pull the wait up.  The order of
  // the updates each entry receives is that of the plain right-looking form.
  double d = readlane_d(a[0], 0) + lambda;
  double dinv = 1.0;  // lane j < NR: 1 / d_j
  double cp[NR], lp = 0.0;
#pragma unroll
  for (int j = 0; j < NR; j++) {
    const double c = l32 > j ? a[j] : 0.0;  // un-normalised column entry of this row; rows <= j are done
    colbuf[j * kCS + l32] = c;
    if (!(d > 0)) ok = false;
    // 1 / d once per column (v_rcp_f64 + two Newton steps, as k_lba_ldlt16 does) instead of a division per row
    double inv = __builtin_amdgcn_rcp(d);
    inv = __builtin_fma(__builtin_fma(-d, inv, 1.0), inv, inv);
    inv = __builtin_fma(__builtin_fma(-d, inv, 1.0), inv, inv);
    dinv = l32 == j ? inv : dinv;
    const double l = c * inv;
    if (j + 1 < NR) {
      const int j1 = j + 1 < NR ? j + 1 : j;
      if (j >= 1) {
        asm volatile("" : "+v"(cp[j1]) : "v"(inv));
        a[j1] = __builtin_fma(-lp, cp[j1], a[j1]);  // pivot j - 1's update of column j + 1
      }
      // column j + 1 is the NEXT broadcast: its update takes A[j+1][j] by v_readlane, so the next ds_write does not wait
      // for this column's trip through LDS
      a[j1] = __builtin_fma(-l, readlane_d(c, j + 1), a[j1]);
      d = readlane_d(a[j1], j + 1) + lambda;  // lane j + 1: its new diagonal
    }
    y = __builtin_fma(-l, readlane_d(y, j), y);
    wave_sync();
    if (j >= 1)
#pragma unroll
      for (int k = j + 2; k < NR; k++) a[k] = __builtin_fma(-lp, cp[k], a[k]);
#pragma unroll
    for (int k = j + 2; k < NR; k++) cp[k] = colbuf[j * kCS + k];
    lp = l;
  }
  if (!ok) return false;
  // TP:backward
  // backward: x_i = (y_i - sum_(j > i) A_ji x_j) / d_i with A_ji = colbuf[i][j] (lane i: its own column, fetched up front)
  double lt[NR];
#pragma unroll
  for (int k = 1; k < NR; k++) lt[k] = colbuf[row * kCS + k] * dinv;
  y *= dinv;
#pragma unroll
  for (int j = NR - 1; j > 0; j--) y = __builtin_fma(-lt[j], readlane_d(y, j), y);
  // TP:write
  if (lane < NR) x[frow] = y;
  wave_sync();
  // the eliminated unknowns: x_(9+t) = (b_(9+t) - off_t x_(24+t)) / d_t
  if (lane < 6) x[9 + lane] = (b[9 + lane] - (NR == 24 ? off * x[24 + lane] : 0.0)) * dbias;
  wave_sync();
  // TP:end
  return true;
}

}  // namespace vieo
