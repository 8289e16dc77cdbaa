// tri_search.hip -- ORBmatcher::SearchForTriangulation (reference src/ORBmatcher.cc:896-1150), a batch of
// neighbours pKF2 of one pKF1 per call; undistorted pinhole key frames and distorted camera rigs.
//   k_tri_points  rigs: K * UnProject(key) of every key once (the image point epipolarConstrain works on)
//   k_tri_gates   one lane per (node-shared key of pKF1) "query": walks the node's keys of pKF2 and keeps the ones
//                 that pass every gate that does not depend on earlier matches -- Hamming <= TH_LOW, the epipole gate
//                 for two monocular keys, GeometricCamera::epipolarConstrain (camera_base.h:287-406, fundamental
//                 matrix branch; Tdata float / Tcalc double as in common/config.h:23-24)
//   host          the reference's loop order over those candidates (tri_walk.h, HIP-free and tested on the CPU): keys of
//                 pKF2 already taken are skipped, best distance (ties to the later key), FillMatchesFromPair, RotHist
//   k_tri_unproject, k_tri_new_points   what LocalMapping::CreateNewMapPoints does with the rows (further down)
// The candidate segment of a query is as long as its node's list in pKF2, so the kernel writes without atomics.
// HBM traffic is the descriptors of both node lists once (32 B per key); the kernel is a gather, latency-bound at
// these sizes (a few thousand queries per neighbour), which is why the neighbours of a key frame go in one launch.
// The host driver (TriCall, at the end) is one call object of two stages, each one pinned block up and one back.
#include <algorithm>
#include <cmath>
#include <vector>

#include "cam_unproject.h"
#include "common.h"
#include "tri_walk.h"
#include "triangulate.h"

namespace vieo {

struct TriPairDev {  // per neighbour
  double F12[4][4][9];  // per (camera of pKF1, camera of pKF2)
  float C2[3];          // pKF1's reference camera centre in pKF2's reference frame (float like the reference)
  float ex, ey;         // its image = the epipole (pinhole: from the host; rig: k_tri_epipole)
  int key_off, feat_off, lvl_off;  // offsets of pKF2's arrays in the concatenated buffers
  int rig;
};

struct TriKfDev {  // per key frame (0 = pKF1, 1 + p = neighbour p)
  vieo_camera cam[4];
  int n_cams, key_off, n_keys, pad;
};

// the image point of every key: the key itself (undistorted), or K * UnProject(key) (bkp_distort, camera_base.h:372-384)
__global__ void __launch_bounds__(64)
k_tri_points(const TriKfDev* __restrict__ kfs, const vieo_keypoint* __restrict__ keys, const uint8_t* __restrict__ key_cam,
             double2* __restrict__ pts, uint8_t* __restrict__ ok) {
  const TriKfDev& K = kfs[blockIdx.y];
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= K.n_keys) return;
  const int g = K.key_off + i;
  const vieo_keypoint kp = keys[g];
  if (K.n_cams == 0) {
    pts[g] = make_double2((double)kp.x, (double)kp.y), ok[g] = 1;
    return;
  }
  CamD c;
  cam_from_abi(K.cam[key_cam[g] & 3], c);
  double X[3];
  cam_unproject(c, kp.x, kp.y, X);
  const double q0 = (c.fx * X[0] + 0.0 * X[1]) + c.cx * X[2], q1 = (0.0 * X[0] + c.fy * X[1]) + c.cy * X[2];
  const double q2 = (0.0 * X[0] + 0.0 * X[1]) + 1.0 * X[2];
  const bool fin = isfinite(q0) && isfinite(q1) && isfinite(q2);
  const double invz = 1. / q2;
  pts[g] = make_double2(q0 * invz, q1 * invz), ok[g] = fin ? 1 : 0;
}

// rigs: pKF2->mpCameras[0]->Project(C2) (ORBmatcher.cc:922-927)
__global__ void k_tri_epipole(TriPairDev* __restrict__ pairs, const TriKfDev* __restrict__ kfs, int n_pairs) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs || !pairs[p].rig) return;
  CamD c;
  cam_from_abi(kfs[1 + p].cam[0], c);
  const double C2[3] = {(double)pairs[p].C2[0], (double)pairs[p].C2[1], (double)pairs[p].C2[2]};
  double uv[2];
  cam_project(c, C2, uv, nullptr);
  pairs[p].ex = (float)uv[0], pairs[p].ey = (float)uv[1];
}

__global__ void __launch_bounds__(64)
k_tri_gates(const TriQuery* __restrict__ queries, int n_queries, const TriPairDev* __restrict__ pairs,
            const vieo_keypoint* __restrict__ keys, const uint8_t* __restrict__ desc, const float* __restrict__ ur,
            const uint8_t* __restrict__ mp, const uint8_t* __restrict__ key_cam, const double2* __restrict__ pts,
            const uint8_t* __restrict__ pt_ok, const int* __restrict__ feat2, const float* __restrict__ scale2,
            const float* __restrict__ sigma2, int only_stereo, int2* __restrict__ cand, int* __restrict__ cand_n) {
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= n_queries) return;
  const TriQuery Q = queries[q];
  const TriPairDev& P = pairs[Q.pair];
  const bool st1 = ur[Q.idx1] >= 0;  // pKF1's keys sit at offset 0
  const uint8_t* d1 = desc + 32 * (size_t)Q.idx1;
  const double2 p1 = pts[Q.idx1];
  const bool ok1 = pt_ok[Q.idx1] != 0;
  const int cam1 = P.rig ? (key_cam[Q.idx1] & 3) : 0;
  int n = 0;
  int2* out = cand + Q.out_off;
  for (int k = 0; k < Q.count2; k++) {
    const int idx2 = feat2[P.feat_off + Q.first2 + k];
    const int g2 = P.key_off + idx2;
    if (mp[g2]) continue;
    const bool st2 = ur[g2] >= 0;
    if (only_stereo && !st2) continue;
    const int dist = hamming256(d1, desc + 32 * (size_t)g2);
    if (dist > kThLow) continue;
    const vieo_keypoint kp2 = keys[g2];
    if (!st1 && !st2) {
      const float distex = P.ex - kp2.x, distey = P.ey - kp2.y;
      if (distex * distex + distey * distey < 100 * scale2[P.lvl_off + kp2.octave]) continue;
    }
    if (!ok1 || !pt_ok[g2]) continue;
    // the epipolar line of key 1 in image 2 (Tdata = float)
    const double* F = P.F12[cam1][P.rig ? (key_cam[g2] & 3) : 0];
    const float a = (float)(p1.x * F[0] + p1.y * F[3] + F[6]);
    const float b = (float)(p1.x * F[1] + p1.y * F[4] + F[7]);
    const float c = (float)(p1.x * F[2] + p1.y * F[5] + F[8]);
    const double2 p2 = pts[g2];
    const float num = (float)((double)a * p2.x + (double)b * p2.y + (double)c);
    const float den = a * a + b * b;
    if (den == 0) continue;
    const float dsqr = num * num / den;
    if (!(dsqr < 3.84f * sigma2[P.lvl_off + kp2.octave])) continue;
    out[n++] = make_int2(idx2, dist);
  }
  cand_n[q] = n;
}

// Tr1r2 = (Tcw1 * Twc2).cast<float>(), T12 = Tcr(cam1) * Tr1r2 * Trc(cam2), F12 = K1^-T [t12]x R12 K2^-1,
// C2 = pKF1's camera centre in pKF2's frame; the epipole of an undistorted pair
static void tri_pair_setup(const vieo_tri_keyframe& A, const vieo_tri_keyframe& B, TriPairDev& P) {
  const bool rig = A.n_cams > 0;
  const int nc1 = rig ? A.n_cams : 1, nc2 = rig ? B.n_cams : 1;
  P.rig = rig ? 1 : 0;
  const double *T1 = A.Tcw, *T2 = B.Tcw;
  double Rr[9], tr[3];
  for (int i = 0; i < 3; i++) {
    double s = 0;
    for (int j = 0; j < 3; j++) {
      double r = 0;
      for (int k = 0; k < 3; k++) r += T1[i * 4 + k] * T2[j * 4 + k];
      Rr[i * 3 + j] = (double)(float)r;
      s += r * T2[j * 4 + 3];
    }
    tr[i] = (double)(float)(T1[i * 4 + 3] - s);
  }
  auto mul = [](const double* X, const double* Y, double* Z) {
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) Z[i * 3 + j] = X[i * 3] * Y[j] + X[i * 3 + 1] * Y[3 + j] + X[i * 3 + 2] * Y[6 + j];
  };
  memset(P.F12, 0, sizeof(P.F12));
  for (int c1 = 0; c1 < nc1; c1++)
    for (int c2 = 0; c2 < nc2; c2++) {
      double R12[9], t12[3];
      if (!rig) {
        memcpy(R12, Rr, 72), memcpy(t12, tr, 24);
      } else {
        const double* Tcr = A.Tcr + 12 * c1;
        const double* Trc = B.Trc + 12 * c2;
        double Ra[9], Rb[9], M[9], v[3];
        for (int i = 0; i < 3; i++)
          for (int j = 0; j < 3; j++) Ra[i * 3 + j] = Tcr[i * 4 + j], Rb[i * 3 + j] = Trc[i * 4 + j];
        mul(Ra, Rr, M), mul(M, Rb, R12);
        for (int i = 0; i < 3; i++) v[i] = tr[i] + (Rr[i * 3] * Trc[3] + Rr[i * 3 + 1] * Trc[7] + Rr[i * 3 + 2] * Trc[11]);
        for (int i = 0; i < 3; i++) t12[i] = Tcr[i * 4 + 3] + (Ra[i * 3] * v[0] + Ra[i * 3 + 1] * v[1] + Ra[i * 3 + 2] * v[2]);
        for (int i = 0; i < 9; i++) R12[i] = (double)(float)R12[i];
        for (int i = 0; i < 3; i++) t12[i] = (double)(float)t12[i];
      }
      const double fx1 = rig ? A.cams[c1].fx : A.fx, fy1 = rig ? A.cams[c1].fy : A.fy;
      const double cx1 = rig ? A.cams[c1].cx : A.cx, cy1 = rig ? A.cams[c1].cy : A.cy;
      const double fx2 = rig ? B.cams[c2].fx : B.fx, fy2 = rig ? B.cams[c2].fy : B.fy;
      const double cx2 = rig ? B.cams[c2].cx : B.cx, cy2 = rig ? B.cams[c2].cy : B.cy;
      const double K1it[9] = {1 / fx1, 0, 0, 0, 1 / fy1, 0, -cx1 / fx1, -cy1 / fy1, 1};
      const double K2i[9] = {1 / fx2, 0, -cx2 / fx2, 0, 1 / fy2, -cy2 / fy2, 0, 0, 1};
      const double H[9] = {0, -t12[2], t12[1], t12[2], 0, -t12[0], -t12[1], t12[0], 0};
      double M1[9], M2[9];
      mul(K1it, H, M1), mul(M1, R12, M2), mul(M2, K2i, P.F12[c1][c2]);
    }
  float R1f[9], t1f[3], R2f[9], t2f[3], Cw[3];
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) R1f[i * 3 + j] = (float)T1[i * 4 + j], R2f[i * 3 + j] = (float)T2[i * 4 + j];
    t1f[i] = (float)T1[i * 4 + 3], t2f[i] = (float)T2[i * 4 + 3];
  }
  for (int i = 0; i < 3; i++)
    Cw[i] = (float)(-((double)R1f[i] * t1f[0] + (double)R1f[3 + i] * t1f[1] + (double)R1f[6 + i] * t1f[2]));
  for (int i = 0; i < 3; i++)
    P.C2[i] = (float)((double)R2f[i * 3] * Cw[0] + (double)R2f[i * 3 + 1] * Cw[1] + (double)R2f[i * 3 + 2] * Cw[2] +
                      (double)t2f[i]);
  P.ex = P.ey = 0;
  if (!rig) {
    const float invz = 1.0f / P.C2[2];
    const float xn = P.C2[0] * invz, yn = P.C2[1] * invz;
    P.ex = (B.fx * xn + 0.0f * yn) + B.cx;
    P.ey = (0.0f * xn + B.fy * yn) + B.cy;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// LocalMapping::CreateNewMapPoints, the part after SearchForTriangulation (reference src/LocalMapping.cc:560-649,
// :690-806): one lane of k_tri_new_points per match row, all neighbours in one launch.
//   k_tri_unproject    UnProject of every key once (a key of pKF1 is in a row of every neighbour)
//   k_tri_new_points   PrepareDatasForTraingulate, the three branches, the distance / far / scale gates
struct TriNewKf {  // per key frame (0 = pKF1, 1 + p = neighbour p)
  CamD cam[4];         // n_cams == 0: cam[0] = the pinhole camera (LocalMapping.cc:715-722)
  double Tcw[4][12];   // Trc(cam)^-1 * Tcw, inverted in double like Twi[i].inverse()
  float Rrc[4][9];     // GetTrc().so3().cast<float>()
  float Rwc[9], Ow[3]; // GetRotation().t() as float, GetCameraCenter()
  float invK[4];       // undistorted: toK().cast<float>().inverse(), its entries (0,0) (0,2) (1,1) (1,2)
  float baseline, bf, scale1;
  int n_cams, key_off, lvl_off, group_off, has_groups;
};

__global__ void __launch_bounds__(64)
k_tri_unproject(const TriNewKf* __restrict__ kfs, const int* __restrict__ n_keys, const vieo_keypoint* __restrict__ keys,
                const uint8_t* __restrict__ key_cam, double2* __restrict__ nrm) {
  const TriNewKf& K = kfs[blockIdx.y];
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n_keys[blockIdx.y]) return;
  const int g = K.key_off + i;
  const vieo_keypoint kp = keys[g];
  double X[3];
  cam_unproject(K.cam[K.n_cams ? (key_cam[g] & 3) : 0], kp.x, kp.y, X);
  nrm[g] = make_double2(X[0], X[1]);
}

struct TriNewArgs {
  const int32_t* rows;      // [n_rows][stride]: the match rows of all neighbours, one after the other
  const int32_t* row_pair;  // [n_rows] the neighbour of each row
  int n_rows, stride;
  const TriNewKf* kfs;
  const vieo_keypoint* keys;  // the buffers of the search: all key frames concatenated at key_off
  const float* uright;
  const uint8_t* key_cam;
  const double2* nrm;
  const float* depth;         // [keys] vdepth_
  const int32_t* key_group;   // [keys] GetMapn2idxs, -1 none
  const double* group_p3d;    // [groups][3] v3dpoints_, all key frames concatenated at group_off
  const float* scale;         // [levels] all key frames concatenated at lvl_off
  const float* sigma2;
  float th_far_pts;
  int8_t* status;  // [n_rows]
  double* x3d;     // [n_rows][3]
  float* x3d_f;    // [n_rows][3]
};

// KeyFrame::UnprojectStereo (KeyFrame.cc:856-888) as the double vector CreateNewMapPoints casts it to; false = NaN
__device__ __forceinline__ bool tri_unproject_stereo(const TriNewArgs& a, const TriNewKf& K, int idx, double* x3d) {
  if (idx < 0) return false;
  const int g = K.key_off + idx;
  const float z = a.depth[g];
  if (!(z > 0)) return false;
  if (K.n_cams > 0) {  // Twc * v3dpoints_[group], cast to float
    const int grp = K.has_groups ? a.key_group[g] : -1;
    if (grp < 0) return false;
    const double* P = a.group_p3d + 3 * (size_t)(K.group_off + grp);
#pragma unroll
    for (int r = 0; r < 3; ++r)
      x3d[r] = (double)(float)((((double)K.Rwc[r * 3] * P[0] + (double)K.Rwc[r * 3 + 1] * P[1]) + (double)K.Rwc[r * 3 + 2] * P[2]) +
                               (double)K.Ow[r]);
    return true;
  }
  const vieo_keypoint kp = a.keys[g];
  const float x = (K.invK[0] * kp.x + K.invK[1]) * z, y = (K.invK[2] * kp.y + K.invK[3]) * z;
#pragma unroll
  for (int r = 0; r < 3; ++r) x3d[r] = (double)(((K.Rwc[r * 3] * x + K.Rwc[r * 3 + 1] * y) + K.Rwc[r * 3 + 2] * z) + K.Ow[r]);
  return true;
}

// N = 2: undistorted key frames (one key per side); N = 8: rigs (one key or -1 per camera of pKF1, then of pKF2)
template <int N>
__global__ void __launch_bounds__(64)
k_tri_new_points(TriNewArgs a) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= a.n_rows) return;
  const int32_t* row = a.rows + (size_t)r * a.stride;
  const TriNewKf& K1 = a.kfs[0];
  const TriNewKf& K2 = a.kfs[1 + a.row_pair[r]];
  const int nc1 = N == 2 ? 1 : K1.n_cams, nc = N == 2 ? 2 : nc1 + K2.n_cams;
  auto get = [&](int s) {
    TriObs o;
    const int idx = s < nc ? row[s] : -1;
    o.on = idx >= 0;
    o.cam = &K1.cam[0], o.Tcw = K1.Tcw[0];  // an empty slot is never read through, but its pointers stay valid
    o.nx = o.ny = 0, o.u = o.v = o.sigma2 = o.uright = o.bf = 0;
    if (o.on) {
      const TriNewKf& K = s < nc1 ? K1 : K2;
      const int g = K.key_off + idx;
      const int cam = K.n_cams ? (a.key_cam[g] & 3) : 0;
      o.cam = &K.cam[cam], o.Tcw = K.Tcw[cam];
      const vieo_keypoint kp = a.keys[g];
      const double2 n = a.nrm[g];
      o.nx = n.x, o.ny = n.y, o.u = kp.x, o.v = kp.y;
      o.sigma2 = a.sigma2[K.lvl_off + kp.octave];
      o.uright = a.uright[g], o.bf = K.bf;
    }
    return o;
  };
  int8_t st = VIEO_NEWPT_NO_KEY;
  double X[3] = {0, 0, 0};
  do {
    // ---- PrepareDatasForTraingulate
    float ray[N][3], rn[N];
    bool on[N];
    // per side (0 = pKF1, 1 = pKF2) in scalars: an array indexed by the side would be indexed at run time
    bool bStereo0 = false, bStereo1 = false, any0 = false, any1 = false;
    float cosSt0 = 1.1f, cosSt1 = 1.1f;
    float smin0 = INFINITY, smin1 = INFINITY, smax0 = -INFINITY, smax1 = -INFINITY;
#pragma unroll
    for (int s = 0; s < N; ++s) {
      const int idx = s < nc ? row[s] : -1;
      on[s] = idx >= 0;
      ray[s][0] = ray[s][1] = ray[s][2] = rn[s] = 0;
      if (!on[s]) continue;
      const bool side = s >= nc1;
      const TriNewKf& K = side ? K2 : K1;
      const int g = K.key_off + idx;
      bool bStereo = side ? bStereo1 : bStereo0;
      float cosSt = side ? cosSt1 : cosSt0;
      if (!bStereo && 0 <= a.uright[g]) bStereo = true;
      if (bStereo) {
        const float c = (float)cos(2 * atan2(K.baseline / 2., (double)a.depth[g]));
        if (cosSt > c) cosSt = c;
      }
      const float sc = a.scale[K.lvl_off + a.keys[g].octave];
      if (side)
        any1 = true, bStereo1 = bStereo, cosSt1 = cosSt, smin1 = fminf(smin1, sc), smax1 = fmaxf(smax1, sc);
      else
        any0 = true, bStereo0 = bStereo, cosSt0 = cosSt, smin0 = fminf(smin0, sc), smax0 = fmaxf(smax0, sc);
      const float* Rc = K.Rrc[K.n_cams ? (a.key_cam[g] & 3) : 0];
      const double2 n = a.nrm[g];
      const float p[3] = {(float)n.x, (float)n.y, 1.0f};
      float xn[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) xn[q] = (Rc[q * 3] * p[0] + Rc[q * 3 + 1] * p[1]) + Rc[q * 3 + 2] * p[2];
#pragma unroll
      for (int q = 0; q < 3; ++q) ray[s][q] = (K.Rwc[q * 3] * xn[0] + K.Rwc[q * 3 + 1] * xn[1]) + K.Rwc[q * 3 + 2] * xn[2];
      rn[s] = sqrtf((ray[s][0] * ray[s][0] + ray[s][1] * ray[s][1]) + ray[s][2] * ray[s][2]);
    }
    if (!any0 || !any1) break;
    float cosRays = 1.1f;
#pragma unroll
    for (int i = 0; i < N - 1; ++i)
#pragma unroll
      for (int j = i + 1; j < N; ++j) {
        if (!(on[i] && on[j] && i < nc1 && j >= nc1)) continue;
        const float c = ((ray[i][0] * ray[j][0] + ray[i][1] * ray[j][1]) + ray[i][2] * ray[j][2]) / (rn[i] * rn[j]);
        if (cosRays > c) cosRays = c;
      }
    // ---- the three branches (LocalMapping.cc:754-779)
    const float cosStereo = fminf(cosSt0, cosSt1);
    bool ok;
    if (cosRays < cosStereo && cosRays > 0 && (bStereo0 || bStereo1 || (double)cosRays < 0.9998)) {
      st = VIEO_NEWPT_DLT;
      ok = triangulate_matches_world<N>(get, (float)(1. - 1e-6), false, X);
    } else if (cosSt0 < cosSt1) {
      st = VIEO_NEWPT_STEREO1;
      ok = tri_unproject_stereo(a, K1, row[0], X) && triangulate_matches_world<N>(get, 1.f, true, X);
    } else if (cosSt1 < cosSt0) {
      st = VIEO_NEWPT_STEREO2;
      ok = tri_unproject_stereo(a, K2, row[nc1], X) && triangulate_matches_world<N>(get, 1.f, true, X);
    } else {
      st = VIEO_NEWPT_LOW_PARALLAX;
      break;
    }
    if (!ok) {
      st = VIEO_NEWPT_TRI_EMPTY;
      break;
    }
    // ---- distances, far points, scale consistency (:781-806)
    const float xf[3] = {(float)X[0], (float)X[1], (float)X[2]};
    const float a1[3] = {xf[0] - K1.Ow[0], xf[1] - K1.Ow[1], xf[2] - K1.Ow[2]};
    const float a2[3] = {xf[0] - K2.Ow[0], xf[1] - K2.Ow[1], xf[2] - K2.Ow[2]};
    const float dist1 = sqrtf((a1[0] * a1[0] + a1[1] * a1[1]) + a1[2] * a1[2]);
    const float dist2 = sqrtf((a2[0] * a2[0] + a2[1] * a2[1]) + a2[2] * a2[2]);
    if (dist1 == 0 || dist2 == 0) {
      st = VIEO_NEWPT_ZERO_DIST;
      break;
    }
    if (a.th_far_pts > 0 && fmaxf(dist1, dist2) >= a.th_far_pts) {
      st = VIEO_NEWPT_FAR;
      break;
    }
    // min / max over the key pairs of scale2 / scale1: the rounded quotient is monotone in both operands
    const float ratioDist = dist2 / dist1, ratioFactor = 1.5f * K1.scale1;
    const float oct0 = smin1 / smax0, oct1 = smax1 / smin0;
    if (ratioDist * ratioFactor < oct1 || ratioDist > oct0 * ratioFactor) st = VIEO_NEWPT_SCALE;
  } while (false);
  const bool acc = st >= 0;
  a.status[r] = st;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    a.x3d[(size_t)r * 3 + q] = acc ? X[q] : 0.0;
    a.x3d_f[(size_t)r * 3 + q] = acc ? (float)X[q] : 0.0f;
  }
}

static void tri_new_kf_setup(const vieo_tri_keyframe& K, const vieo_tri_stereo& S, TriNewKf& d) {
  memset((void*)&d, 0, sizeof(d));
  const int nc = K.n_cams > 0 ? K.n_cams : 1;
  for (int c = 0; c < nc; c++) {
    double Ri[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, ti[3] = {0, 0, 0};
    if (K.n_cams > 0) {
      cam_from_abi(K.cams[c], d.cam[c]);
      const double* Trc = K.Trc + 12 * c;
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Ri[i * 3 + j] = Trc[j * 4 + i], d.Rrc[c][i * 3 + j] = (float)Trc[i * 4 + j];
      for (int i = 0; i < 3; i++) ti[i] = -((Ri[i * 3] * Trc[3] + Ri[i * 3 + 1] * Trc[7]) + Ri[i * 3 + 2] * Trc[11]);
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 4; j++)
          d.Tcw[c][i * 4 + j] = ((Ri[i * 3] * K.Tcw[j] + Ri[i * 3 + 1] * K.Tcw[4 + j]) + Ri[i * 3 + 2] * K.Tcw[8 + j]) +
                                (j == 3 ? ti[i] : 0.0);
    } else {
      CamD& cd = d.cam[0];
      cd.fx = K.fx, cd.fy = K.fy, cd.cx = K.cx, cd.cy = K.cy, cd.bf = 0, cd.model = VIEO_CAM_PINHOLE, cd.num_k = 0;
      d.Rrc[0][0] = d.Rrc[0][4] = d.Rrc[0][8] = 1.0f;
      memcpy(d.Tcw[0], K.Tcw, sizeof(d.Tcw[0]));
    }
  }
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) d.Rwc[i * 3 + j] = (float)K.Tcw[j * 4 + i];
    d.Ow[i] = S.Ow[i];
  }
  // Eigen's 3x3 inverse: cofactors times 1 / det, in float
  const float invdet = 1.0f / (K.fx * K.fy);
  d.invK[0] = K.fy * invdet, d.invK[1] = -(K.fy * K.cx) * invdet, d.invK[2] = K.fx * invdet, d.invK[3] = -(K.fx * K.cy) * invdet;
  d.baseline = S.baseline, d.bf = S.bf, d.scale1 = K.n_levels > 1 ? K.scale_factor[1] : K.scale_factor[0];
  d.n_cams = K.n_cams;
}

static bool tri_cam_ok(const vieo_camera& c) {
  CamD d;
  return cam_from_abi(c, d);
}

static_assert(sizeof(TriCand) == sizeof(int2), "k_tri_gates writes int2 (idx2, dist)");

namespace {

// One call of any of the three entries: the plan (tri_walk.h), then up to two stages, each one pinned block up, its
// launches on the null stream and one copy back.  Every array lies at the plan's offsets in both stages, so the
// triangulation that follows a search in one call reads the keys, uright, key cameras and level tables the search sent.
struct TriCall {
  TriPlan plan;
  std::vector<int> n_groups;
  TriRows rows;
  Staging S, T;  // the search's block, the triangulation's
  struct Shared {  // what both stages read, on the device; null until a stage of THIS call has staged it
    const vieo_keypoint* keys;
    const float* ur;
    const uint8_t* kc;
    const float *scale, *sigma2;
  } dv = {};
  struct SharedOffs {
    size_t keys, ur, kc, scale, sigma2;
  };

  size_t n_keys() const { return (size_t)std::max(plan.key_off.back(), 1); }
  SharedOffs reserve_shared(Staging& B) const {
    const size_t ka = n_keys(), lvls = (size_t)plan.lvl_off.back() * 4;
    return {B.in(nullptr, ka * sizeof(vieo_keypoint)), B.in(nullptr, ka * 4), B.in(nullptr, ka), B.in(nullptr, lvls), B.in(nullptr, lvls)};
  }
  // after B.alloc(); the key cameras of an undistorted key frame are zero
  void write_shared(const TriArgs& a, Staging& B, const SharedOffs& o) {
    for (int f = 0; f <= a.n_kf2; f++) {
      const vieo_tri_keyframe& K = a.kf(f);
      const size_t nk = K.n_keys, off = plan.key_off[f];
      memcpy(B.hw<float>(o.scale) + plan.lvl_off[f], K.scale_factor, (size_t)K.n_levels * 4);
      memcpy(B.hw<float>(o.sigma2) + plan.lvl_off[f], K.level_sigma2, (size_t)K.n_levels * 4);
      if (!nk) continue;
      memcpy(B.hw<vieo_keypoint>(o.keys) + off, K.keys, nk * sizeof(vieo_keypoint));
      memcpy(B.hw<float>(o.ur) + off, K.uright, nk * 4);
      if (K.n_cams > 0)
        memcpy(B.hw<uint8_t>(o.kc) + off, K.key_cam, nk);
      else
        memset(B.hw<uint8_t>(o.kc) + off, 0, nk);
    }
    dv = Shared{B.d<vieo_keypoint>(o.keys), B.d<float>(o.ur), B.d<uint8_t>(o.kc), B.d<float>(o.scale), B.d<float>(o.sigma2)};
  }

  int run(const TriArgs& a) {
    dv = Shared{};
    int rc = tri_check(a, tri_cam_ok, n_groups);
    if (rc != VIEO_OK || a.n_kf2 == 0) return rc;
    if ((rc = require_device()) != VIEO_OK) return rc;
    tri_layout(a, n_groups, plan);
    if (a.search) {
      tri_queries(a, plan);
      if ((rc = search(a)) != VIEO_OK) return rc;
    }
    return a.tri ? triangulate(a) : VIEO_OK;
  }

  int search(const TriArgs& a) {
    const int n = a.n_kf2, nq = (int)plan.queries.size();
    if (nq == 0) return tri_walk(a, plan, nullptr, nullptr);
    S.reset();
    const size_t ka = n_keys();
    const size_t o_q = S.in(nullptr, nq * sizeof(TriQuery)), o_pairs = S.in(nullptr, n * sizeof(TriPairDev));
    const size_t o_kfs = S.in(nullptr, (1 + n) * sizeof(TriKfDev));
    const SharedOffs o_sh = reserve_shared(S);
    const size_t o_desc = S.in(nullptr, ka * 32), o_mp = S.in(nullptr, ka);
    const size_t o_f2 = S.in(nullptr, (size_t)std::max(plan.feat_off.back(), 1) * 4);
    const size_t o_cn = S.out((size_t)nq * 4), o_cand = S.out(std::max<size_t>(plan.n_cand, 1) * sizeof(int2));
    const size_t o_pts = S.scratch(ka * sizeof(double2)), o_ok = S.scratch(ka);
    int rc = S.alloc();
    if (rc != VIEO_OK) return rc;
    memcpy(S.hw<TriQuery>(o_q), plan.queries.data(), nq * sizeof(TriQuery));
    write_shared(a, S, o_sh);
    for (int f = 0; f <= n; f++) {
      const vieo_tri_keyframe& K = a.kf(f);
      const size_t nk = K.n_keys, off = plan.key_off[f];
      TriKfDev& d = S.hw<TriKfDev>(o_kfs)[f];
      memset(&d, 0, sizeof(d));
      for (int c = 0; c < K.n_cams; c++) d.cam[c] = K.cams[c];
      d.n_cams = K.n_cams, d.key_off = (int)off, d.n_keys = K.n_keys;
      if (nk) memcpy(S.hw<uint8_t>(o_desc) + 32 * off, K.descriptors, nk * 32), memcpy(S.hw<uint8_t>(o_mp) + off, K.has_mappoint, nk);
      if (f == 0) continue;
      TriPairDev& P = S.hw<TriPairDev>(o_pairs)[f - 1];
      tri_pair_setup(*a.kf1, K, P);
      P.key_off = (int)off, P.feat_off = plan.feat_off[f], P.lvl_off = plan.lvl_off[f];
      const size_t nf = plan.feat_off[f + 1] - plan.feat_off[f];
      if (nf) memcpy(S.hw<int>(o_f2) + P.feat_off, K.node_feat, nf * 4);
    }
    if ((rc = S.upload(nullptr)) != VIEO_OK) return rc;
    hipLaunchKernelGGL(k_tri_points, dim3((plan.max_keys + 63) / 64, 1 + n), dim3(64), 0, nullptr, S.d<TriKfDev>(o_kfs), dv.keys, dv.kc,
                       S.d<double2>(o_pts), S.d<uint8_t>(o_ok));
    hipLaunchKernelGGL(k_tri_epipole, dim3((n + 63) / 64), dim3(64), 0, nullptr, S.d<TriPairDev>(o_pairs), S.d<TriKfDev>(o_kfs), n);
    hipLaunchKernelGGL(k_tri_gates, dim3((nq + 63) / 64), dim3(64), 0, nullptr, S.d<TriQuery>(o_q), nq, S.d<TriPairDev>(o_pairs),
                       dv.keys, S.d<uint8_t>(o_desc), dv.ur, S.d<uint8_t>(o_mp), dv.kc, S.d<double2>(o_pts), S.d<uint8_t>(o_ok),
                       S.d<int>(o_f2), dv.scale, dv.sigma2, a.only_stereo, S.d<int2>(o_cand), S.d<int>(o_cn));
    VIEO_HIP_CHECK(hipGetLastError());
    if ((rc = S.download(o_cn, nullptr)) != VIEO_OK) return rc;
    return tri_walk(a, plan, (const TriCand*)S.h(o_cand), (const int*)S.h(o_cn));
  }

  int triangulate(const TriArgs& a) {
    int rc = tri_gather(a, rows);
    const int n_rows = rows.n(), nf = 1 + a.n_kf2;
    if (rc != VIEO_OK || n_rows == 0) return rc;
    T.reset();
    const size_t ka = n_keys(), groups = plan.group_off.back();
    const size_t o_kfs = T.in(nullptr, nf * sizeof(TriNewKf)), o_nk = T.in(nullptr, (size_t)nf * 4);
    const size_t o_rows = T.in(rows.rows.data(), rows.rows.size() * 4), o_rp = T.in(rows.row_pair.data(), (size_t)n_rows * 4);
    const size_t o_depth = T.in(nullptr, ka * 4), o_grp = T.in(nullptr, groups ? ka * 4 : 0), o_p3d = T.in(nullptr, groups * 24);
    const bool alone = !dv.keys;  // no search in this call has staged the shared arrays
    const SharedOffs o_sh = alone ? reserve_shared(T) : SharedOffs{};
    const size_t o_st = T.out(n_rows), o_x3d = T.out((size_t)n_rows * 24), o_x3df = T.out((size_t)n_rows * 12);
    const size_t o_nrm = T.scratch(ka * sizeof(double2));
    if ((rc = T.alloc()) != VIEO_OK) return rc;
    if (alone) write_shared(a, T, o_sh);
    if (groups) std::fill_n(T.hw<int32_t>(o_grp), ka, -1);
    for (int f = 0; f < nf; f++) {
      const vieo_tri_keyframe& K = a.kf(f);
      const vieo_tri_stereo& St = a.st(f);
      const size_t nk = K.n_keys, off = plan.key_off[f];
      TriNewKf& d = T.hw<TriNewKf>(o_kfs)[f];
      tri_new_kf_setup(K, St, d);
      d.key_off = (int)off, d.lvl_off = plan.lvl_off[f], d.group_off = plan.group_off[f], d.has_groups = n_groups[f] > 0;
      T.hw<int>(o_nk)[f] = K.n_keys;
      if (n_groups[f]) memcpy(T.hw<double>(o_p3d) + 3 * (size_t)d.group_off, St.group_p3d, (size_t)n_groups[f] * 24);
      if (nk) memcpy(T.hw<float>(o_depth) + off, St.depth, nk * 4);
      if (nk && n_groups[f]) memcpy(T.hw<int32_t>(o_grp) + off, St.key_group, nk * 4);
    }
    if ((rc = T.upload(nullptr)) != VIEO_OK) return rc;
    hipLaunchKernelGGL(k_tri_unproject, dim3((plan.max_keys + 63) / 64, nf), dim3(64), 0, nullptr, T.d<TriNewKf>(o_kfs), T.d<int>(o_nk),
                       dv.keys, dv.kc, T.d<double2>(o_nrm));
    TriNewArgs k;
    k.rows = T.d<int32_t>(o_rows), k.row_pair = T.d<int32_t>(o_rp), k.n_rows = n_rows, k.stride = a.pair_stride;
    k.kfs = T.d<TriNewKf>(o_kfs), k.keys = dv.keys, k.uright = dv.ur, k.key_cam = dv.kc;
    k.nrm = T.d<double2>(o_nrm), k.depth = T.d<float>(o_depth), k.key_group = T.d<int32_t>(o_grp);
    k.group_p3d = T.d<double>(o_p3d), k.scale = dv.scale, k.sigma2 = dv.sigma2;
    k.th_far_pts = a.th_far_pts, k.status = T.d<int8_t>(o_st), k.x3d = T.d<double>(o_x3d), k.x3d_f = T.d<float>(o_x3df);
    if (a.kf1->n_cams > 0)
      hipLaunchKernelGGL(k_tri_new_points<8>, dim3((n_rows + 63) / 64), dim3(64), 0, nullptr, k);
    else
      hipLaunchKernelGGL(k_tri_new_points<2>, dim3((n_rows + 63) / 64), dim3(64), 0, nullptr, k);
    VIEO_HIP_CHECK(hipGetLastError());
    if ((rc = T.download(o_st, nullptr)) != VIEO_OK) return rc;
    tri_scatter(a, rows, (const int8_t*)T.h(o_st), (const double*)T.h(o_x3d), (const float*)T.h(o_x3df));
    return VIEO_OK;
  }
};
thread_local TriCall g_tri;

}  // namespace

}  // namespace vieo

using namespace vieo;

extern "C" int vieo_search_for_triangulation(const vieo_tri_keyframe* kf1, const vieo_tri_keyframe* kf2s, int n_kf2,
                                             int only_stereo, int check_orientation, int32_t pair_capacity,
                                             int32_t pair_stride, int32_t* h_pairs, int32_t* h_n_pairs,
                                             int32_t* h_n_matches) {
  TriArgs a{};
  a.search = true, a.kf1 = kf1, a.kf2s = kf2s, a.n_kf2 = n_kf2, a.only_stereo = only_stereo, a.check_orientation = check_orientation;
  a.pair_capacity = pair_capacity, a.pair_stride = pair_stride;
  a.h_pairs = h_pairs, a.h_n_pairs = h_n_pairs, a.h_n_matches = h_n_matches;
  return g_tri.run(a);
}

extern "C" int vieo_triangulate_new_points(const vieo_tri_keyframe* kf1, const vieo_tri_stereo* st1,
                                           const vieo_tri_keyframe* kf2s, const vieo_tri_stereo* st2s, int n_kf2,
                                           float th_far_pts, int32_t pair_capacity, int32_t pair_stride,
                                           const int32_t* h_pairs, const int32_t* h_n_pairs, int8_t* h_status,
                                           double* h_x3d, float* h_x3d_f, int32_t* h_n_new) {
  TriArgs a{};
  a.tri = true, a.kf1 = kf1, a.kf2s = kf2s, a.st1 = st1, a.st2s = st2s, a.n_kf2 = n_kf2, a.th_far_pts = th_far_pts;
  a.pair_capacity = pair_capacity, a.pair_stride = pair_stride, a.rows = h_pairs, a.n_rows = h_n_pairs;
  a.h_status = h_status, a.h_x3d = h_x3d, a.h_x3d_f = h_x3d_f, a.h_n_new = h_n_new;
  return g_tri.run(a);
}

extern "C" int vieo_create_new_map_points(const vieo_tri_keyframe* kf1, const vieo_tri_stereo* st1,
                                          const vieo_tri_keyframe* kf2s, const vieo_tri_stereo* st2s, int n_kf2,
                                          int only_stereo, int check_orientation, float th_far_pts,
                                          int32_t pair_capacity, int32_t pair_stride, int32_t* h_pairs,
                                          int32_t* h_n_pairs, int32_t* h_n_matches, int8_t* h_status, double* h_x3d,
                                          float* h_x3d_f, int32_t* h_n_new) {
  TriArgs a{};
  a.search = a.tri = true, a.kf1 = kf1, a.kf2s = kf2s, a.st1 = st1, a.st2s = st2s, a.n_kf2 = n_kf2;
  a.only_stereo = only_stereo, a.check_orientation = check_orientation, a.th_far_pts = th_far_pts;
  a.pair_capacity = pair_capacity, a.pair_stride = pair_stride;
  a.h_pairs = h_pairs, a.h_n_pairs = h_n_pairs, a.h_n_matches = h_n_matches, a.rows = h_pairs, a.n_rows = h_n_pairs;
  a.h_status = h_status, a.h_x3d = h_x3d, a.h_x3d_f = h_x3d_f, a.h_n_new = h_n_new;
  return g_tri.run(a);
}
