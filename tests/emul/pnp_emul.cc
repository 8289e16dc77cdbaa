// Host build of vieo_slam_amd/csrc/pnp_device.h (test only): the lane functions of the two PnP kernels as ordinary C++,
// one hypothesis in lane 0 of a [element][lane] work area, so the device's arithmetic (Jacobi eigen-solver, Householder
// least squares, polar factor, CheckInliers) can be compared with the numpy restatement without a GPU.
// The helpers have entry points of their own (tests/test_solver_algebra.py), and pnp_epnp can run in any lane of the work
// area and hand out the values that decide its branches (PNP_TAP; the slots are listed in
// tests/hip_unit/solver_algebra_test.hip).
#include <vector>

static double* g_pnp_tap = nullptr;  // 48 doubles of the call in progress, or none
#define PNP_TAP(slot, value) \
  if (g_pnp_tap) g_pnp_tap[slot] = (value);

#include "../../vieo_slam_amd/csrc/pnp_device.h"

extern "C" {

// EPnP over the correspondences idx[0..cnt) of Xw[n][3] / uv[n][2]; K = fx, fy, cx, cy.  Rt[12] = R row-major, then t.
void emul_pnp_epnp(const float* Xw, const float* uv, int n, const float* K, const int* idx, int cnt, double* Rt) {
  using namespace vieo;
  std::vector<double> sA(144 * kPnpLanes, 0.0), sV(144 * kPnpLanes, 0.0);
  const PnpCandDev C{0, n, K[0], K[1], K[2], K[3], (n + 63) / 64, 0};
  double R[3][3], t[3];
  pnp_epnp(C, Xw, uv, idx, cnt, sA.data(), sV.data(), 0, R, t);
  pnp_store_pose(R, t, Rt);
}

// CheckInliers at Rt over all n correspondences; mask[(n + 63) / 64]; returns the count
int emul_pnp_check(const float* Xw, const float* uv, const float* max_err, int n, const float* K, const double* Rt,
                   unsigned long long* mask) {
  using namespace vieo;
  const PnpCandDev C{0, n, K[0], K[1], K[2], K[3], (n + 63) / 64, 0};
  double R[3][3], t[3];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) R[r][c] = Rt[3 * r + c];
    t[r] = Rt[9 + r];
  }
  return pnp_check_inliers(C, Xw, uv, max_err, R, t, mask);
}

// pnp_epnp in lane `lane` of a work area whose other lanes hold `fill`; tap[48] may be null
void emul_pnp_epnp_lane(const float* Xw, const float* uv, int n, const float* K, const int* idx, int cnt, int lane,
                        double fill, double* Rt, double* tap) {
  using namespace vieo;
  std::vector<double> sA(144 * kPnpLanes, fill), sV(144 * kPnpLanes, fill);
  const PnpCandDev C{0, n, K[0], K[1], K[2], K[3], (n + 63) / 64, 0};
  double R[3][3], t[3];
  g_pnp_tap = tap;
  pnp_epnp(C, Xw, uv, idx, cnt, sA.data(), sV.data(), lane, R, t);
  g_pnp_tap = nullptr;
  pnp_store_pose(R, t, Rt);
}

// pnp_lstsq6<nc> on A[6][nc] (row-major) and b[6]; nc = 3, 4 or 5
int emul_pnp_lstsq6(int nc, const double* A, const double* b, double* x) {
  using namespace vieo;
  double bb[6];
  for (int r = 0; r < 6; r++) bb[r] = b[r];
#define EMUL_LSTSQ(NC)                                            \
  if (nc == NC) {                                                 \
    double M[6][NC], xx[NC];                                      \
    for (int r = 0; r < 6; r++)                                   \
      for (int c = 0; c < NC; c++) M[r][c] = A[r * NC + c];       \
    pnp_lstsq6<NC>(M, bb, xx);                                    \
    for (int c = 0; c < NC; c++) x[c] = xx[c];                    \
    return 0;                                                     \
  }
  EMUL_LSTSQ(3)
  EMUL_LSTSQ(4)
  EMUL_LSTSQ(5)
#undef EMUL_LSTSQ
  return 1;
}

void emul_pnp_rot(const double* abg, double* tcs) { vieo::pnp_rot(abg[0], abg[1], abg[2], tcs[0], tcs[1], tcs[2]); }

void emul_pnp_eig3(const double* S, double* d, double* U) {
  double M[3][3], dd[3], UU[3][3];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) M[r][c] = S[3 * r + c];
  vieo::pnp_eig3(M, dd, UU);
  for (int r = 0; r < 3; r++) {
    d[r] = dd[r];
    for (int c = 0; c < 3; c++) U[3 * r + c] = UU[r][c];
  }
}

void emul_pnp_polar3(const double* B, double* R) {
  double M[3][3], RR[3][3];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) M[r][c] = B[3 * r + c];
  vieo::pnp_polar3(M, RR);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) R[3 * r + c] = RR[r][c];
}

// frame[12] = c0, ci row-major
void emul_pnp_alphas(const double* frame, const float* X, double* a) {
  vieo::PnpFrame F;
  for (int r = 0; r < 3; r++) {
    F.c0[r] = frame[r];
    for (int c = 0; c < 3; c++) F.ci[r][c] = frame[3 + 3 * r + c];
  }
  vieo::pnp_alphas(F, X, a);
}

void emul_pnp_project(const float* K, const double* Rt, const float* X, double* uv) {
  using namespace vieo;
  const PnpCandDev C{0, 1, K[0], K[1], K[2], K[3], 1, 0};
  double R[3][3], t[3];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) R[r][c] = Rt[3 * r + c];
    t[r] = Rt[9 + r];
  }
  pnp_project(C, R, t, X, uv[0], uv[1]);
}

}  // extern "C"
