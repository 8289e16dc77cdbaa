// Host build of the rig instances of the two PnP kernels (test only): vieo_slam_amd/csrc/pnp_device.h with RIG = true and
// pnp_usun.h as ordinary C++, one hypothesis in lane 0 of a [element][lane] work area, so usun, the rig EPnP and the rig
// CheckInliers of the device can be compared with the numpy restatement (tests/reloc_rig_ref.py) without a GPU.
#include <cstring>
#include <vector>

#include "../../vieo_slam_amd/csrc/pnp_usun.h"

namespace {

bool rig_record(const vieo_pnp_rig* R, vieo::PnpRigDev& D) {
  if (R->n_cams < 1 || R->n_cams > 4) return false;
  D.n_cams = R->n_cams, D.reserved = 0;
  for (int c = 0; c < R->n_cams; c++) {
    if (!vieo::cam_from_abi(R->cams[c], D.cams[c])) return false;
    std::memcpy(D.Tcr[c], R->Tcr[c], sizeof(D.Tcr[c]));
    std::memcpy(D.Trc[c], R->Trc[c], sizeof(D.Trc[c]));
  }
  return true;
}

}  // namespace

extern "C" {

// usun[n][2] of uv[n][2] / cam_of[n]; K = fx, fy, cx, cy of camera 0.  returns 0, or -1 for a bad rig
int emul_pnp_rig_usun(const vieo_pnp_rig* rig, const float* uv, const unsigned char* cam_of, int n, const float* K,
                      double* usun) {
  vieo::PnpRigDev D;
  if (!rig_record(rig, D)) return -1;
  for (int i = 0; i < n; i++)
    if (cam_of[i] >= D.n_cams) return -1;
  for (int i = 0; i < n; i++) vieo::pnp_usun(D, cam_of[i], uv[2 * i], uv[2 * i + 1], K[0], K[1], K[2], K[3], usun + 2 * i);
  return 0;
}

// rig EPnP over the correspondences idx[0..cnt) of Xw[n][3] / uv[n][2] / cam_of[n] (usun computed here).  Rt[12]
int emul_pnp_rig_epnp(const vieo_pnp_rig* rig, const float* Xw, const float* uv, const unsigned char* cam_of, int n,
                      const float* K, const int* idx, int cnt, double* Rt) {
  using namespace vieo;
  PnpRigDev D;
  std::vector<double> usun(2 * (size_t)n + 2);
  if (emul_pnp_rig_usun(rig, uv, cam_of, n, K, usun.data()) != 0 || !rig_record(rig, D)) return -1;
  std::vector<double> sA(144 * kPnpLanes, 0.0), sV(144 * kPnpLanes, 0.0);
  const PnpCandDev C{0, n, K[0], K[1], K[2], K[3], (n + 63) / 64, 0};
  const PnpRigArgs G{&D, cam_of, usun.data()};
  double R[3][3], t[3];
  pnp_epnp_t<true>(C, G, Xw, uv, idx, cnt, sA.data(), sV.data(), 0, R, t);
  pnp_store_pose(R, t, Rt);
  return 0;
}

// rig CheckInliers at Rt over all n correspondences; mask[(n + 63) / 64]; returns the count, -1 for a bad rig
int emul_pnp_rig_check(const vieo_pnp_rig* rig, const float* Xw, const float* uv, const unsigned char* cam_of,
                       const float* max_err, int n, const float* K, const double* Rt, unsigned long long* mask) {
  using namespace vieo;
  PnpRigDev D;
  if (!rig_record(rig, D)) return -1;
  for (int i = 0; i < n; i++)
    if (cam_of[i] >= D.n_cams) return -1;
  const PnpCandDev C{0, n, K[0], K[1], K[2], K[3], (n + 63) / 64, 0};
  const PnpRigArgs G{&D, cam_of, nullptr};
  double R[3][3], t[3];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) R[r][c] = Rt[3 * r + c];
    t[r] = Rt[9 + r];
  }
  return pnp_check_inliers_t<true>(C, G, Xw, uv, max_err, R, t, mask);
}

}  // extern "C"
