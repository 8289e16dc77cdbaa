// Host build of vieo_slam_amd/csrc/pnp_device.h (test only): the lane functions of the two PnP kernels as ordinary C++,
// one hypothesis in lane 0 of a [element][lane] work area, so the device's arithmetic (Jacobi eigen-solver, Householder
// least squares, polar factor, CheckInliers) can be compared with the numpy restatement without a GPU.
#include <vector>

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

}  // extern "C"
