// Host build of vieo_slam_amd/csrc/sim3_solver_device.h (test only): the lane functions of k_sim3_hypotheses as ordinary
// C++, so the device's arithmetic (Horn's closed form with its Jacobi eigen-solver, CheckInliers) can be compared with
// the numpy restatement without a GPU.
#include "../../vieo_slam_amd/csrc/sim3_solver_device.h"

extern "C" {

// ComputeSim3 on the 3 pairs P1[3][3] / P2[3][3] (one point per row).  sRt[13] = R row-major, t, s.
void emul_sim3_horn(const float* P1, const float* P2, int fix_scale, double* sRt) {
  using namespace vieo;
  double A[3][3], B[3][3], R[3][3], t[3], s;
  for (int i = 0; i < 3; i++)
    for (int c = 0; c < 3; c++) A[i][c] = (double)P1[3 * i + c], B[i][c] = (double)P2[3 * i + c];
  s3s_horn(A, B, fix_scale != 0, R, t, s);
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) sRt[3 * r + c] = R[r][c];
    sRt[9 + r] = t[r];
  }
  sRt[12] = s;
}

// CheckInliers at sRt over n correspondences; mask[(n + 63) / 64]; returns the count
int emul_sim3_check(const float* X1, const float* X2, const int* max_err1, const int* max_err2, const int* cam1,
                    const int* cam2, int n, const vieo_camera* cams1, const vieo_camera* cams2, const double* sRt,
                    unsigned long long* mask) {
  using namespace vieo;
  double R[3][3], t[3];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) R[r][c] = sRt[3 * r + c];
    t[r] = sRt[9 + r];
  }
  Sim3Pose T;
  s3s_pose(R, t, sRt[12], T);
  int count = 0;
  for (int w = 0; w < (n + 63) / 64; w++) mask[w] = 0;
  for (int i = 0; i < n; i++) {
    CamD c1, c2;
    cam_from_abi(cams1[cam1[i]], c1), cam_from_abi(cams2[cam2[i]], c2);
    if (s3s_is_inlier(T, c1, c2, X1 + 3 * i, X2 + 3 * i, (float)max_err1[i], (float)max_err2[i]))
      mask[i / 64] |= 1ull << (i % 64), ++count;
  }
  return count;
}

}  // extern "C"
