// The lane functions of vieo_imu_init (vieo_slam_amd/csrc/imu_init_device.h) compiled for the host: the gyro edge and
// its Gauss-Newton step, the rows, the Jacobi SVD solve, the gravity frame and steps 1-4 as a whole with a functor of 1 or
// 64 lanes (64: the lane <-> row map of the kernels and the adjacent-pair tree of their DPP sums).  Test only.
//
// The SO(3) closed forms below restate vieo_slam_amd/csrc/imu_device.h (device-only there) line by line for the host; on
// the device imu_init_device.h uses the originals, which the GPU parity tests cover.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/vieo_hot.h"

namespace vieo {
struct Qd {
  double w, x, y, z;
};
static inline Qd q_norm(Qd q) {
  const double r = 1.0 / sqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
  return Qd{q.w * r, q.x * r, q.y * r, q.z * r};
}
static inline Qd q_mul(const Qd& a, const Qd& b) {
  return Qd{a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
            a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z, a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x};
}
static inline Qd q_conj(const Qd& q) { return Qd{q.w, -q.x, -q.y, -q.z}; }
static inline void q_to_R(const Qd& s, double* R) {
  const double tx = 2 * s.x, ty = 2 * s.y, tz = 2 * s.z;
  const double twx = tx * s.w, twy = ty * s.w, twz = tz * s.w;
  const double txx = tx * s.x, txy = ty * s.x, txz = tz * s.x;
  const double tyy = ty * s.y, tyz = tz * s.y, tzz = tz * s.z;
  R[0] = 1 - (tyy + tzz), R[1] = txy - twz, R[2] = txz + twy;
  R[3] = txy + twz, R[4] = 1 - (txx + tzz), R[5] = tyz - twx;
  R[6] = txz - twy, R[7] = tyz + twx, R[8] = 1 - (txx + tyy);
}
static inline Qd R_to_q(const double* R) {
  Qd q;
  double t = R[0] + R[4] + R[8];
  if (t > 0) {
    t = sqrt(t + 1.0);
    q.w = 0.5 * t;
    t = 0.5 / t;
    q.x = (R[7] - R[5]) * t, q.y = (R[2] - R[6]) * t, q.z = (R[3] - R[1]) * t;
  } else {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[i * 3 + i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = sqrt(R[i * 3 + i] - R[j * 3 + j] - R[k * 3 + k] + 1.0);
    double v[3];
    v[i] = 0.5 * t;
    t = 0.5 / t;
    q.w = (R[k * 3 + j] - R[j * 3 + k]) * t;
    v[j] = (R[j * 3 + i] + R[i * 3 + j]) * t;
    v[k] = (R[k * 3 + i] + R[i * 3 + k]) * t;
    q.x = v[0], q.y = v[1], q.z = v[2];
  }
  return q_norm(q);
}
static inline Qd so3_exp_q(const double* w) {
  const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  double imag, real;
  if (th < 1e-5) {
    const double t2 = th * th;
    imag = 0.5 - t2 / 48., real = 1.0 - t2 / 8.;
  } else {
    const double h = 0.5 * th;
    imag = sin(h) / th, real = cos(h);
  }
  return q_norm(Qd{real, imag * w[0], imag * w[1], imag * w[2]});
}
static inline void so3_log_q(const Qd& q, double* out) {
  const double n = sqrt(q.x * q.x + q.y * q.y + q.z * q.z), w = q.w, sw = w * w;
  double f;
  if (n < 1e-5) {
    f = 2. / w - 2. / 3 * (n * n) / (w * sw);
  } else if (fabs(w) < 1e-5) {
    f = (w > 0 ? M_PI : -M_PI) / n;
    const double n2 = n * n, n4 = n2 * n2;
    f -= 2 * w / n2 - 2. / 3 * (w * sw) / n4;
  } else
    f = 2 * atan(n / w) / n;
  out[0] = f * q.x, out[1] = f * q.y, out[2] = f * q.z;
}
static inline void hat3(const double* w, double* O) {
  O[0] = 0, O[1] = -w[2], O[2] = w[1], O[3] = w[2], O[4] = 0, O[5] = -w[0], O[6] = -w[1], O[7] = w[0], O[8] = 0;
}
static inline void mm3(const double* A, const double* B, double* C) {
  double t[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) t[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
  for (int i = 0; i < 9; i++) C[i] = t[i];
}
static inline void mv3(const double* A, const double* v, double* r) {
  const double a = A[0] * v[0] + A[1] * v[1] + A[2] * v[2], b = A[3] * v[0] + A[4] * v[1] + A[5] * v[2],
               c = A[6] * v[0] + A[7] * v[1] + A[8] * v[2];
  r[0] = a, r[1] = b, r[2] = c;
}
static inline void so3_JrInv_d(const double* w, double* J) {
  const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  double O[9], O2[9];
  hat3(w, O);
  if (th < 1e-5) {
    mm3(O, O, O2);
    for (int i = 0; i < 9; i++) J[i] = ((i % 4) == 0 ? 1.0 : 0.0) + 0.5 * O[i] + (1. / 12.) * O2[i];
  } else {
    const double k[3] = {w[0] / th, w[1] / th, w[2] / th};
    double K[9];
    hat3(k, K);
    mm3(K, K, O2);
    const double sth = sin(th), cth = cos(th);
    const double c = 1.0 - (1.0 + cth) * th / (2.0 * sth);
    for (int i = 0; i < 9; i++) J[i] = ((i % 4) == 0 ? 1.0 : 0.0) + 0.5 * O[i] + c * O2[i];
  }
}
}  // namespace vieo

#include "../../vieo_slam_amd/csrc/imu_init_device.h"

using namespace vieo;

namespace {

template <int NL>
struct HostLanes {
  template <int N, class F>
  void run(F f, double* out) {
    static double part[NL][N];
    for (int l = 0; l < NL; l++) f(l, NL, part[l]);
    for (int w = 1; w < NL; w *= 2)
      for (int l = 0; l < NL; l += 2 * w)
        for (int i = 0; i < N; i++) part[l][i] += part[l + w][i];
    for (int i = 0; i < N; i++) out[i] = part[0][i];
  }
  void sync() {}
};

IiSeq view(int n, const double* Twc, const void* pre, const double* prv, const double* Rcb, const double* pcb, double G) {
  IiSeq S;
  S.Twc = Twc, S.pre = (const vieo_imu_preint*)pre, S.prv = prv, S.n = n, S.G = G;
  memcpy(S.Rcb, Rcb, sizeof(S.Rcb)), memcpy(S.pcb, pcb, sizeof(S.pcb));
  return S;
}

template <class L>
int jacobi(L& lanes, int nc, double* M, int m, double* x, double* w) {
  return nc == 4 ? ii_jacobi_solve<4>(lanes, M, m, m, x, w) : ii_jacobi_solve<6>(lanes, M, m, m, x, w);
}

}  // namespace

extern "C" {

int emul_ii_max_sweeps() { return VIEO_IMU_INIT_MAX_SWEEPS; }

void emul_ii_gyro_edge(const double* Rcb, const double* Twc_i, const double* Twc_j, const void* pre, const double* prv,
                       double* e, double* J, double* W) {
  ii_gyro_edge(Rcb, Twc_i, Twc_j, *(const vieo_imu_preint*)pre, prv, e, J, W);
}

// rows: m x (nc + 1) row-major, nc = 4 or 6; returns the sweeps
int emul_ii_jacobi(int n_lanes, int m, int nc, const double* rows, double* x, double* w) {
  std::vector<double> M((size_t)m * (nc + 1));
  for (int r = 0; r < m; r++)
    for (int c = 0; c <= nc; c++) M[(size_t)c * m + r] = rows[(size_t)r * (nc + 1) + c];
  if (n_lanes == 64) {
    HostLanes<64> L;
    return jacobi(L, nc, M.data(), m, x, w);
  }
  HostLanes<1> L;
  return jacobi(L, nc, M.data(), m, x, w);
}

int emul_ii_gravity_frame(const double* gw_star, double* RwI) { return ii_gravity_frame(gw_star, RwI) ? 1 : 0; }

// steps 1 (on pre0 / prv0) and 3-4 (on pre1) of one sequence; rows1 [3 (n - 2)][5] / rows2 [..][7] (row-major, may be
// NULL): the matrices as they were filled
void emul_ii_steps(int n_lanes, int n, const double* Twc, const void* pre0, const double* prv0, const void* pre1,
                   const double* Rcb, const double* pcb, double G, vieo_imu_init_result* out, double* rows1, double* rows2) {
  vieo_imu_init_result R;
  memset(&R, 0, sizeof(R));
  *out = R;
  if (n < 4) {
    out->status = VIEO_IMU_INIT_FEW_KF;
    return;
  }
  const int m = 3 * (n - 2);
  std::vector<double> M((size_t)7 * m);
  const IiSeq S0 = view(n, Twc, pre0, prv0, Rcb, pcb, G), S1 = view(n, Twc, pre1, nullptr, Rcb, pcb, G);
  auto go = [&](auto& L) {
    ii_gyro_step(L, S0, R.bg, &R.n_eq_gyro);
    if (rows1) {
      ii_fill_first(L, S1, M.data(), m);
      for (int r = 0; r < m; r++)
        for (int c = 0; c < 5; c++) rows1[5 * r + c] = M[(size_t)c * m + r];
    }
    ii_solve(L, S1, M.data(), m, R);
    if (rows2 && R.status == VIEO_IMU_INIT_OK) {
      ii_fill_second(L, S1, R.RwI, M.data(), m);
      for (int r = 0; r < m; r++)
        for (int c = 0; c < 7; c++) rows2[7 * r + c] = M[(size_t)c * m + r];
    }
  };
  if (n_lanes == 64) {
    HostLanes<64> L;
    go(L);
  } else {
    HostLanes<1> L;
    go(L);
  }
  *out = R;
}

// step 5's closed forms for one key frame i with successor j (or, last != 0, predecessor i - 1 = `Twc_o`)
void emul_ii_apply_kf(const double* Twc, const double* Twc_o, int last, const double* Rcb, const double* pcb, double s,
                      const double* gw, const void* pre, double* Tcw, double* p, double* q, double* v) {
  const vieo_imu_preint& M = *(const vieo_imu_preint*)pre;
  double Rwb[9];
  ii_scaled_Tcw(Twc, s, Tcw);
  ii_nav_pose(Twc, Rcb, pcb, s, p, q, Rwb);
  if (!last)
    ii_velocity(Twc, Twc_o, Rcb, pcb, s, gw, M.dt, M.pij, v);
  else {
    double vp[3], Rp[9], Rpb[9], r[3];
    ii_velocity(Twc_o, Twc, Rcb, pcb, s, gw, M.dt, M.pij, vp);
    ii_Rwc(Twc_o, Rp);
    mm3(Rp, Rcb, Rpb);
    mv3(Rpb, M.vij, r);
    for (int j = 0; j < 3; j++) v[j] = vp[j] + gw[j] * M.dt + r[j];
  }
}

}  // extern "C"
