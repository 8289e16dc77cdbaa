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

// ---- the helpers by themselves (tests/test_solver_algebra.py)
void emul_s3s_top_eigenvector(const double* N, double* q) {
  double M[4][4], qq[4];
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) M[r][c] = N[4 * r + c];
  vieo::s3s_top_eigenvector(M, qq);
  for (int k = 0; k < 4; k++) q[k] = qq[k];
}

// s3s_horn on double points (one per row); sRt[13] = R row-major, t, s
void emul_s3s_horn(const double* P1, const double* P2, int fix_scale, double* sRt) {
  double A[3][3], B[3][3], R[3][3], t[3], s;
  for (int i = 0; i < 3; i++)
    for (int c = 0; c < 3; c++) A[i][c] = P1[3 * i + c], B[i][c] = P2[3 * i + c];
  vieo::s3s_horn(A, B, fix_scale != 0, R, t, s);
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) sRt[3 * r + c] = R[r][c];
    sRt[9 + r] = t[r];
  }
  sRt[12] = s;
}

static void pose_in(const double* T24, vieo::Sim3Pose& T) {
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) T.A12[r][c] = T24[3 * r + c], T.A21[r][c] = T24[12 + 3 * r + c];
    T.t12[r] = T24[9 + r], T.t21[r] = T24[21 + r];
  }
}

// T24 = A12[9], t12[3], A21[9], t21[3]
void emul_s3s_pose(const double* sRt, double* T24) {
  double R[3][3], t[3];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) R[r][c] = sRt[3 * r + c];
    t[r] = sRt[9 + r];
  }
  vieo::Sim3Pose T;
  vieo::s3s_pose(R, t, sRt[12], T);
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) T24[3 * r + c] = T.A12[r][c], T24[12 + 3 * r + c] = T.A21[r][c];
    T24[9 + r] = T.t12[r], T24[21 + r] = T.t21[r];
  }
}

// a camera is f[25] = fx, fy, cx, cy, bf, Rcb[9], tcb[3], k[8] and i[2] = model, num_k
static vieo::CamD cam_in(const double* f, const int* i) {
  vieo::CamD d;
  d.fx = f[0], d.fy = f[1], d.cx = f[2], d.cy = f[3], d.bf = f[4];
  for (int k = 0; k < 9; k++) d.Rcb[k] = f[5 + k];
  for (int k = 0; k < 3; k++) d.tcb[k] = f[14 + k];
  for (int k = 0; k < 8; k++) d.k[k] = f[17 + k];
  d.model = i[0], d.num_k = i[1];
  return d;
}

// At[12] = A row-major, t; has_A = 0: the point itself
void emul_s3s_project(const double* cam_f, const int* cam_i, int has_A, const double* At, const float* X, float* uv) {
  const vieo::CamD cam = cam_in(cam_f, cam_i);
  double A[3][3];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) A[r][c] = At[3 * r + c];
  if (has_A)
    vieo::s3s_project(cam, A, At + 9, X, uv);
  else
    vieo::s3s_project(cam, nullptr, nullptr, X, uv);
}

float emul_s3s_dist2(const float* ab) { return vieo::s3s_dist2(ab, ab + 2); }

int emul_s3s_is_inlier(const double* T24, const double* cam1_f, const int* cam1_i, const double* cam2_f, const int* cam2_i,
                       const float* X12, const float* me) {
  vieo::Sim3Pose T;
  pose_in(T24, T);
  return vieo::s3s_is_inlier(T, cam_in(cam1_f, cam1_i), cam_in(cam2_f, cam2_i), X12, X12 + 3, me[0], me[1]) ? 1 : 0;
}

}  // extern "C"
