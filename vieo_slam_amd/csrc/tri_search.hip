// tri_search.hip -- ORBmatcher::SearchForTriangulation (reference src/ORBmatcher.cc:896-1150), a batch of
// neighbours pKF2 of one pKF1 per call; undistorted pinhole key frames and distorted camera rigs.
//   k_tri_points  rigs: K * UnProject(key) of every key once (the image point epipolarConstrain works on)
//   k_tri_gates   one lane per (node-shared key of pKF1) "query": walks the node's keys of pKF2 and keeps the ones
//                 that pass every gate that does not depend on earlier matches -- Hamming <= TH_LOW, the epipole gate
//                 for two monocular keys, GeometricCamera::epipolarConstrain (camera_base.h:287-406, fundamental
//                 matrix branch; Tdata float / Tcalc double as in common/config.h:23-24)
//   host          the reference's loop order over those candidates: keys of pKF2 already taken are skipped, best
//                 distance (ties to the later key), FillMatchesFromPair (match_groups.h), RotHist (bow_walk.h)
//   k_tri_unproject, k_tri_new_points   what LocalMapping::CreateNewMapPoints does with the rows (further down)
// The candidate segment of a query is as long as its node's list in pKF2, so the kernel writes without atomics.
// HBM traffic is the descriptors of both node lists once (32 B per key); the kernel is a gather, latency-bound at
// these sizes (a few thousand queries per neighbour), which is why the neighbours of a key frame go in one launch.
#include <algorithm>
#include <cmath>
#include <vector>

#include "bow_walk.h"
#include "cam_unproject.h"
#include "common.h"
#include "match_groups.h"
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

struct TriQuery {
  int idx1, pair, first2, count2, out_off;
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

static bool tri_kf_ok(const vieo_tri_keyframe& K) {
  if (K.n_keys < 0 || K.n_nodes < 0 || K.n_levels <= 0 || !K.scale_factor || !K.level_sigma2) return false;
  if (K.n_keys > 0 && (!K.keys || !K.descriptors || !K.uright || !K.has_mappoint)) return false;
  if (K.n_cams < 0 || K.n_cams > 4 || (K.n_cams > 0 && (!K.cams || !K.Tcr || !K.Trc || (K.n_keys > 0 && !K.key_cam)))) return false;
  if (!node_table_ok(K.n_keys, K.n_nodes, K.node_id, K.node_first, K.node_feat)) return false;
  for (int i = 0; i < K.n_keys; i++)
    if (K.keys[i].octave < 0 || K.keys[i].octave >= K.n_levels || (K.n_cams > 0 && K.key_cam[i] >= K.n_cams)) return false;
  for (int c = 0; c < K.n_cams; c++) {
    CamD d;
    if (!cam_from_abi(K.cams[c], d)) return false;
  }
  return true;
}

struct TriScratch {
  DevBuf q, pairs, kfs, k, d, u, m, kc, pts, ok, f2, s2, g2, cand, cn;
};
static thread_local TriScratch g_tri;

// skip[p] != 0 (may be null): neighbour p is not searched (CreateNewMapPoints' baseline test), its counts are 0.
// *resident (may be null): whether the keys, uright and key cameras of all key frames were left in g_tri's buffers.
static int tri_search_impl(const vieo_tri_keyframe* kf1, const vieo_tri_keyframe* kf2s, int n_kf2, int only_stereo,
                           int check_orientation, int32_t pair_capacity, int32_t pair_stride, int32_t* h_pairs,
                           int32_t* h_n_pairs, int32_t* h_n_matches, const uint8_t* skip, bool* resident) {
  if (resident) *resident = false;
  if (!kf1 || !kf2s || n_kf2 <= 0 || pair_capacity < 0 || (pair_capacity > 0 && !h_pairs) || !h_n_pairs || !h_n_matches)
    return VIEO_E_INVALID;
  if (!tri_kf_ok(*kf1)) {
    set_error("SearchForTriangulation: pKF1 is inconsistent (nodes ascending, feature / camera indices and octaves in range)");
    return VIEO_E_INVALID;
  }
  const vieo_tri_keyframe& A = *kf1;
  const int nc1 = A.n_cams > 0 ? A.n_cams : 1;
  for (int p = 0; p < n_kf2; p++) {
    if (!tri_kf_ok(kf2s[p])) {
      set_error("SearchForTriangulation: neighbour %d is inconsistent", p);
      return VIEO_E_INVALID;
    }
    if ((kf2s[p].n_cams > 0) != (A.n_cams > 0)) {  // assert(!usedistort[1]) / assert(usedistort[1]), ORBmatcher.cc:949,952
      set_error("SearchForTriangulation: neighbour %d and pKF1 are not of one kind (undistorted / rig)", p);
      return VIEO_E_INVALID;
    }
    if (pair_stride < nc1 + (kf2s[p].n_cams > 0 ? kf2s[p].n_cams : 1)) {
      set_error("SearchForTriangulation: pair_stride %d is smaller than the cameras of pair %d", pair_stride, p);
      return VIEO_E_INVALID;
    }
  }
  int rc = require_device();
  if (rc != VIEO_OK) return rc;
  // ---- queries in the reference's order (shared nodes ascending, keys of pKF1 in the node's order)
  std::vector<TriPairDev> pairs(n_kf2);
  std::vector<TriKfDev> kfd(1 + n_kf2);
  std::vector<TriQuery> queries;
  std::vector<int> q_begin(n_kf2 + 1, 0);
  size_t keys_all = A.n_keys, feats2 = 0, lvls2 = 0, n_cand = 0;
  int max_keys = A.n_keys;
  auto fill_kf = [](const vieo_tri_keyframe& K, int key_off, TriKfDev& d) {
    memset(&d, 0, sizeof(d));
    for (int c = 0; c < K.n_cams; c++) d.cam[c] = K.cams[c];
    d.n_cams = K.n_cams, d.key_off = key_off, d.n_keys = K.n_keys;
  };
  fill_kf(A, 0, kfd[0]);
  for (int p = 0; p < n_kf2; p++) {
    const vieo_tri_keyframe& B = kf2s[p];
    tri_pair_setup(A, B, pairs[p]);
    pairs[p].key_off = (int)keys_all, pairs[p].feat_off = (int)feats2, pairs[p].lvl_off = (int)lvls2;
    fill_kf(B, (int)keys_all, kfd[1 + p]);
    keys_all += B.n_keys, feats2 += B.n_nodes ? B.node_first[B.n_nodes] : 0, lvls2 += B.n_levels;
    max_keys = std::max(max_keys, B.n_keys);
    q_begin[p] = (int)queries.size();
    if (skip && skip[p]) continue;
    for_shared_nodes(A.node_id, A.n_nodes, B.node_id, B.n_nodes, [&](int n1, int n2) {
      const int first2 = B.node_first[n2], count2 = B.node_first[n2 + 1] - first2;
      for (int i1 = A.node_first[n1]; i1 < A.node_first[n1 + 1] && count2 > 0; i1++) {
        const int idx1 = A.node_feat[i1];
        if (A.has_mappoint[idx1] || (only_stereo && !(A.uright[idx1] >= 0))) continue;
        queries.push_back({idx1, p, first2, count2, (int)n_cand});
        n_cand += count2;
      }
    });
  }
  q_begin[n_kf2] = (int)queries.size();
  const int nq = (int)queries.size();
  std::vector<int> cand_n(nq, 0);
  std::vector<int2> cand(std::max<size_t>(n_cand, 1));
  if (nq > 0) {
    TriScratch& S = g_tri;
    const size_t ka = std::max<size_t>(keys_all, 1);
    if ((rc = S.q.ensure(nq * sizeof(TriQuery))) != VIEO_OK || (rc = S.pairs.ensure(n_kf2 * sizeof(TriPairDev))) != VIEO_OK ||
        (rc = S.kfs.ensure((1 + n_kf2) * sizeof(TriKfDev))) != VIEO_OK ||
        (rc = S.k.ensure(ka * sizeof(vieo_keypoint))) != VIEO_OK || (rc = S.d.ensure(ka * 32)) != VIEO_OK ||
        (rc = S.u.ensure(ka * 4)) != VIEO_OK || (rc = S.m.ensure(ka)) != VIEO_OK || (rc = S.kc.ensure(ka)) != VIEO_OK ||
        (rc = S.pts.ensure(ka * sizeof(double2))) != VIEO_OK || (rc = S.ok.ensure(ka)) != VIEO_OK ||
        (rc = S.f2.ensure(std::max<size_t>(feats2, 1) * 4)) != VIEO_OK || (rc = S.s2.ensure(lvls2 * 4)) != VIEO_OK ||
        (rc = S.g2.ensure(lvls2 * 4)) != VIEO_OK || (rc = S.cand.ensure(cand.size() * sizeof(int2))) != VIEO_OK ||
        (rc = S.cn.ensure(nq * 4)) != VIEO_OK)
      return rc;
    VIEO_HIP_CHECK(hipMemcpy(S.q.p, queries.data(), nq * sizeof(TriQuery), hipMemcpyHostToDevice));
    VIEO_HIP_CHECK(hipMemcpy(S.pairs.p, pairs.data(), n_kf2 * sizeof(TriPairDev), hipMemcpyHostToDevice));
    VIEO_HIP_CHECK(hipMemcpy(S.kfs.p, kfd.data(), (1 + n_kf2) * sizeof(TriKfDev), hipMemcpyHostToDevice));
    for (int f = 0; f <= n_kf2; f++) {
      const vieo_tri_keyframe& K = f == 0 ? A : kf2s[f - 1];
      const size_t nk = K.n_keys, off = kfd[f].key_off;
      if (!nk) continue;
      VIEO_HIP_CHECK(hipMemcpy(S.k.as<vieo_keypoint>() + off, K.keys, nk * sizeof(vieo_keypoint), hipMemcpyHostToDevice));
      VIEO_HIP_CHECK(hipMemcpy(S.d.as<uint8_t>() + 32 * off, K.descriptors, nk * 32, hipMemcpyHostToDevice));
      VIEO_HIP_CHECK(hipMemcpy(S.u.as<float>() + off, K.uright, nk * 4, hipMemcpyHostToDevice));
      VIEO_HIP_CHECK(hipMemcpy(S.m.as<uint8_t>() + off, K.has_mappoint, nk, hipMemcpyHostToDevice));
      if (K.n_cams > 0)
        VIEO_HIP_CHECK(hipMemcpy(S.kc.as<uint8_t>() + off, K.key_cam, nk, hipMemcpyHostToDevice));
      else
        VIEO_HIP_CHECK(hipMemset(S.kc.as<uint8_t>() + off, 0, nk));
    }
    for (int p = 0; p < n_kf2; p++) {
      const vieo_tri_keyframe& B = kf2s[p];
      const TriPairDev& P = pairs[p];
      const size_t nf = B.n_nodes ? B.node_first[B.n_nodes] : 0;
      if (nf) VIEO_HIP_CHECK(hipMemcpy(S.f2.as<int>() + P.feat_off, B.node_feat, nf * 4, hipMemcpyHostToDevice));
      VIEO_HIP_CHECK(hipMemcpy(S.s2.as<float>() + P.lvl_off, B.scale_factor, (size_t)B.n_levels * 4, hipMemcpyHostToDevice));
      VIEO_HIP_CHECK(hipMemcpy(S.g2.as<float>() + P.lvl_off, B.level_sigma2, (size_t)B.n_levels * 4, hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL(k_tri_points, dim3((std::max(max_keys, 1) + 63) / 64, 1 + n_kf2), dim3(64), 0, nullptr,
                       S.kfs.as<TriKfDev>(), S.k.as<vieo_keypoint>(), S.kc.as<uint8_t>(), S.pts.as<double2>(), S.ok.as<uint8_t>());
    hipLaunchKernelGGL(k_tri_epipole, dim3((n_kf2 + 63) / 64), dim3(64), 0, nullptr, S.pairs.as<TriPairDev>(),
                       S.kfs.as<TriKfDev>(), n_kf2);
    hipLaunchKernelGGL(k_tri_gates, dim3((nq + 63) / 64), dim3(64), 0, nullptr, S.q.as<TriQuery>(), nq,
                       S.pairs.as<TriPairDev>(), S.k.as<vieo_keypoint>(), S.d.as<uint8_t>(), S.u.as<float>(),
                       S.m.as<uint8_t>(), S.kc.as<uint8_t>(), S.pts.as<double2>(), S.ok.as<uint8_t>(), S.f2.as<int>(),
                       S.s2.as<float>(), S.g2.as<float>(), only_stereo, S.cand.as<int2>(), S.cn.as<int>());
    VIEO_HIP_CHECK(hipGetLastError());
    VIEO_HIP_CHECK(hipMemcpy(cand_n.data(), S.cn.p, nq * 4, hipMemcpyDeviceToHost));
    VIEO_HIP_CHECK(hipMemcpy(cand.data(), S.cand.p, cand.size() * sizeof(int2), hipMemcpyDeviceToHost));
    if (resident) *resident = true;
  }
  // ---- the order-dependent part, per neighbour (ORBmatcher.cc:962-1146)
  FeGroups G;
  for (int p = 0; p < n_kf2; p++) {
    const vieo_tri_keyframe& B = kf2s[p];
    const bool rig = A.n_cams > 0;
    const int nc2 = rig ? B.n_cams : 1, nc = nc1 + nc2;
    int32_t nk[8];
    for (int c = 0; c < nc; c++) nk[c] = c < nc1 ? A.n_keys : B.n_keys;  // tables indexed by the key's global index
    G.reset(nc, nk);
    RotHist rot;
    int nmatches = 0;
    for (int q = q_begin[p]; q < q_begin[p + 1]; q++) {
      const TriQuery& Q = queries[q];
      const int cam1 = rig ? A.key_cam[Q.idx1] : 0;
      int bestDist[4] = {kThLow, kThLow, kThLow, kThLow}, bestIdx2[4] = {-1, -1, -1, -1};  // per image
      for (int k = 0; k < cand_n[q]; k++) {
        const int2 c = cand[Q.out_off + k];
        const int img = rig ? B.key_cam[c.x] : 0;
        const int g = G.key2g[nc1 + img][c.x];
        if (g >= 0 && G.idxs[(size_t)g * nc + cam1] != -1) continue;  // pKF2's key already matched to this camera
        if (c.y > bestDist[img]) continue;
        bestIdx2[img] = c.x, bestDist[img] = c.y;
      }
      for (int img = 0; img < nc2; img++) {
        if (bestIdx2[img] < 0) continue;
        if (fe_fill(G, cam1, Q.idx1, nc1 + img, bestIdx2[img], (float)bestDist[img], true, nullptr)) ++nmatches;
        if (check_orientation) {
          const int bin = rot_bin(A.keys[Q.idx1].angle, B.keys[bestIdx2[img]].angle);
          if (bin < 0 || bin >= kHistoLen) {
            set_error("SearchForTriangulation: key angles outside [0, 360)");
            return VIEO_E_INVALID;
          }
          rot.push(bin, Q.idx1);
        }
      }
    }
    if (check_orientation)
      rot.finish([&](int idx1) {
        const int g = G.key2g[rig ? A.key_cam[idx1] : 0][idx1];
        if (g < 0) return;
        G.good[g] = 0;
        nmatches--;
      });
    int np = 0;
    for (int g = 0; g < G.size(); g++) {
      int cnt = 0;
      for (int c = 0; c < nc; c++) cnt += G.idxs[(size_t)g * nc + c] != -1;
      if (cnt < 2 || !G.good[g]) continue;
      if (np < pair_capacity) {
        int32_t* row = h_pairs + ((size_t)p * pair_capacity + np) * pair_stride;
        for (int c = 0; c < pair_stride; c++) row[c] = c < nc ? G.idxs[(size_t)g * nc + c] : -1;
      }
      np++;
    }
    h_n_pairs[p] = np, h_n_matches[p] = nmatches;
    if (np > pair_capacity) {
      set_error("SearchForTriangulation: neighbour %d has %d matches, capacity %d", p, np, pair_capacity);
      return VIEO_E_CAPACITY;
    }
  }
  return VIEO_OK;
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

struct TriNewScratch {
  DevBuf kfs, nk, rows, rp, nrm, depth, grp, p3d, scale, sigma2, st, x3d, x3df;
};
static thread_local TriNewScratch g_tri_new;

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

static bool tri_stereo_ok(const vieo_tri_keyframe& K, const vieo_tri_stereo& S, int* n_groups) {
  *n_groups = 0;
  if (K.n_keys > 0 && !S.depth) return false;
  if (K.n_cams > 0 && S.key_group)
    for (int i = 0; i < K.n_keys; i++) {
      if (S.key_group[i] < -1) return false;
      *n_groups = std::max(*n_groups, S.key_group[i] + 1);
    }
  return *n_groups == 0 || S.group_p3d;
}

// the baseline test of LocalMapping.cc:691-698 (stereo / RGB-D / rigs)
static bool tri_baseline_short(const vieo_tri_stereo& s1, const vieo_tri_stereo& s2) {
  const float v[3] = {s2.Ow[0] - s1.Ow[0], s2.Ow[1] - s1.Ow[1], s2.Ow[2] - s1.Ow[2]};
  return std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) < s2.baseline;
}

static int tri_new_check(const vieo_tri_keyframe* kf1, const vieo_tri_stereo* st1, const vieo_tri_keyframe* kf2s,
                         const vieo_tri_stereo* st2s, int n_kf2, int32_t pair_capacity, int32_t pair_stride,
                         std::vector<int>& n_groups) {
  n_groups.assign(1 + n_kf2, 0);
  if (!tri_kf_ok(*kf1) || !tri_stereo_ok(*kf1, *st1, &n_groups[0])) {
    set_error("CreateNewMapPoints: pKF1 is inconsistent");
    return VIEO_E_INVALID;
  }
  const int nc1 = kf1->n_cams > 0 ? kf1->n_cams : 1;
  for (int p = 0; p < n_kf2; p++) {
    if (!tri_kf_ok(kf2s[p]) || !tri_stereo_ok(kf2s[p], st2s[p], &n_groups[1 + p])) {
      set_error("CreateNewMapPoints: neighbour %d is inconsistent", p);
      return VIEO_E_INVALID;
    }
    if ((kf2s[p].n_cams > 0) != (kf1->n_cams > 0)) {
      set_error("CreateNewMapPoints: neighbour %d and pKF1 are not of one kind (undistorted / rig)", p);
      return VIEO_E_INVALID;
    }
    if (pair_stride < nc1 + (kf2s[p].n_cams > 0 ? kf2s[p].n_cams : 1)) {
      set_error("CreateNewMapPoints: pair_stride %d is smaller than the cameras of pair %d", pair_stride, p);
      return VIEO_E_INVALID;
    }
  }
  return VIEO_OK;
}

// resident: the search of this call left keys / uright / key cameras in g_tri (same offsets as computed here)
static int tri_new_points_impl(const vieo_tri_keyframe* kf1, const vieo_tri_stereo* st1, const vieo_tri_keyframe* kf2s,
                               const vieo_tri_stereo* st2s, int n_kf2, float th_far_pts, int32_t pair_capacity,
                               int32_t pair_stride, const int32_t* h_pairs, const int32_t* h_n_pairs,
                               const std::vector<int>& n_groups, bool resident, int8_t* h_status, double* h_x3d,
                               float* h_x3d_f, int32_t* h_n_new) {
  const vieo_tri_keyframe& A = *kf1;
  const bool rig = A.n_cams > 0;
  const int nc1 = rig ? A.n_cams : 1;
  // ---- the rows of the neighbours that pass the baseline test, one after the other
  std::vector<int32_t> rows, row_pair;
  std::vector<size_t> row_dst;
  for (int p = 0; p < n_kf2; p++) {
    h_n_new[p] = 0;
    const int np = h_n_pairs[p];
    if (np < 0) {
      set_error("CreateNewMapPoints: neighbour %d has a negative row count", p);
      return VIEO_E_INVALID;
    }
    if (np > pair_capacity) {
      set_error("CreateNewMapPoints: neighbour %d has %d rows, capacity %d", p, np, pair_capacity);
      return VIEO_E_CAPACITY;
    }
    const vieo_tri_keyframe& B = kf2s[p];
    const int nc = nc1 + (rig ? B.n_cams : 1);
    const bool skip = tri_baseline_short(*st1, st2s[p]);
    for (int m = 0; m < np; m++) {
      const size_t at = (size_t)p * pair_capacity + m;
      const int32_t* row = h_pairs + at * pair_stride;
      if (skip) {
        h_status[at] = VIEO_NEWPT_SKIPPED;
        for (int q = 0; q < 3; q++) h_x3d[at * 3 + q] = 0, h_x3d_f[at * 3 + q] = 0;
        continue;
      }
      for (int c = 0; c < nc; c++)
        if (row[c] < -1 || row[c] >= (c < nc1 ? A.n_keys : B.n_keys)) {
          set_error("CreateNewMapPoints: row %d of neighbour %d holds key %d", m, p, row[c]);
          return VIEO_E_INVALID;
        }
      for (int c = 0; c < pair_stride; c++) rows.push_back(c < nc ? row[c] : -1);
      row_pair.push_back(p), row_dst.push_back(at);
    }
  }
  const int n_rows = (int)row_pair.size();
  if (n_rows == 0) return VIEO_OK;
  // ---- per key frame records and the concatenated side arrays
  std::vector<TriNewKf> kfd(1 + n_kf2);
  std::vector<int> nkeys(1 + n_kf2);
  size_t keys_all = 0, lvls = 0, groups = 0;
  int max_keys = 1;
  for (int f = 0; f <= n_kf2; f++) {
    const vieo_tri_keyframe& K = f == 0 ? A : kf2s[f - 1];
    tri_new_kf_setup(K, f == 0 ? *st1 : st2s[f - 1], kfd[f]);
    kfd[f].key_off = (int)keys_all, kfd[f].lvl_off = (int)lvls, kfd[f].group_off = (int)groups;
    kfd[f].has_groups = n_groups[f] > 0;
    nkeys[f] = K.n_keys, keys_all += K.n_keys, lvls += K.n_levels, groups += n_groups[f];
    max_keys = std::max(max_keys, K.n_keys);
  }
  TriScratch& S = g_tri;
  TriNewScratch& T = g_tri_new;
  const size_t ka = std::max<size_t>(keys_all, 1);
  int rc;
  if ((rc = T.kfs.ensure(kfd.size() * sizeof(TriNewKf))) != VIEO_OK || (rc = T.nk.ensure(nkeys.size() * 4)) != VIEO_OK ||
      (rc = T.rows.ensure(rows.size() * 4)) != VIEO_OK || (rc = T.rp.ensure((size_t)n_rows * 4)) != VIEO_OK ||
      (rc = T.nrm.ensure(ka * sizeof(double2))) != VIEO_OK || (rc = T.depth.ensure(ka * 4)) != VIEO_OK ||
      (rc = T.grp.ensure(ka * 4)) != VIEO_OK || (rc = T.p3d.ensure(std::max<size_t>(groups, 1) * 24)) != VIEO_OK ||
      (rc = T.scale.ensure(lvls * 4)) != VIEO_OK || (rc = T.sigma2.ensure(lvls * 4)) != VIEO_OK ||
      (rc = T.st.ensure(n_rows)) != VIEO_OK || (rc = T.x3d.ensure((size_t)n_rows * 24)) != VIEO_OK ||
      (rc = T.x3df.ensure((size_t)n_rows * 12)) != VIEO_OK)
    return rc;
  if (!resident &&
      ((rc = S.k.ensure(ka * sizeof(vieo_keypoint))) != VIEO_OK || (rc = S.u.ensure(ka * 4)) != VIEO_OK ||
       (rc = S.kc.ensure(ka)) != VIEO_OK))
    return rc;
  VIEO_HIP_CHECK(hipMemcpy(T.kfs.p, kfd.data(), kfd.size() * sizeof(TriNewKf), hipMemcpyHostToDevice));
  VIEO_HIP_CHECK(hipMemcpy(T.nk.p, nkeys.data(), nkeys.size() * 4, hipMemcpyHostToDevice));
  VIEO_HIP_CHECK(hipMemcpy(T.rows.p, rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
  VIEO_HIP_CHECK(hipMemcpy(T.rp.p, row_pair.data(), (size_t)n_rows * 4, hipMemcpyHostToDevice));
  // the side arrays of all key frames go up concatenated, one copy per array (a copy per key frame and array was
  // most of the call's time)
  std::vector<float> h_depth(ka), h_scale(lvls), h_sigma2(lvls), h_ur(resident ? 0 : ka);
  std::vector<int32_t> h_grp(groups ? ka : 0, -1);
  std::vector<double> h_p3d(groups * 3);
  std::vector<vieo_keypoint> h_keys(resident ? 0 : ka);
  std::vector<uint8_t> h_kc(resident ? 0 : ka, 0);
  for (int f = 0; f <= n_kf2; f++) {
    const vieo_tri_keyframe& K = f == 0 ? A : kf2s[f - 1];
    const vieo_tri_stereo& St = f == 0 ? *st1 : st2s[f - 1];
    const size_t nk = K.n_keys, off = kfd[f].key_off;
    memcpy(h_scale.data() + kfd[f].lvl_off, K.scale_factor, (size_t)K.n_levels * 4);
    memcpy(h_sigma2.data() + kfd[f].lvl_off, K.level_sigma2, (size_t)K.n_levels * 4);
    if (n_groups[f]) memcpy(h_p3d.data() + 3 * (size_t)kfd[f].group_off, St.group_p3d, (size_t)n_groups[f] * 24);
    if (!nk) continue;
    memcpy(h_depth.data() + off, St.depth, nk * 4);
    if (n_groups[f]) memcpy(h_grp.data() + off, St.key_group, nk * 4);
    if (resident) continue;
    memcpy(h_keys.data() + off, K.keys, nk * sizeof(vieo_keypoint));
    memcpy(h_ur.data() + off, K.uright, nk * 4);
    if (K.n_cams > 0) memcpy(h_kc.data() + off, K.key_cam, nk);
  }
  VIEO_HIP_CHECK(hipMemcpy(T.scale.p, h_scale.data(), lvls * 4, hipMemcpyHostToDevice));
  VIEO_HIP_CHECK(hipMemcpy(T.sigma2.p, h_sigma2.data(), lvls * 4, hipMemcpyHostToDevice));
  VIEO_HIP_CHECK(hipMemcpy(T.depth.p, h_depth.data(), ka * 4, hipMemcpyHostToDevice));
  if (groups) {
    VIEO_HIP_CHECK(hipMemcpy(T.grp.p, h_grp.data(), ka * 4, hipMemcpyHostToDevice));
    VIEO_HIP_CHECK(hipMemcpy(T.p3d.p, h_p3d.data(), groups * 24, hipMemcpyHostToDevice));
  }
  if (!resident) {
    VIEO_HIP_CHECK(hipMemcpy(S.k.p, h_keys.data(), ka * sizeof(vieo_keypoint), hipMemcpyHostToDevice));
    VIEO_HIP_CHECK(hipMemcpy(S.u.p, h_ur.data(), ka * 4, hipMemcpyHostToDevice));
    VIEO_HIP_CHECK(hipMemcpy(S.kc.p, h_kc.data(), ka, hipMemcpyHostToDevice));
  }
  hipLaunchKernelGGL(k_tri_unproject, dim3((max_keys + 63) / 64, 1 + n_kf2), dim3(64), 0, nullptr, T.kfs.as<TriNewKf>(),
                     T.nk.as<int>(), S.k.as<vieo_keypoint>(), S.kc.as<uint8_t>(), T.nrm.as<double2>());
  TriNewArgs a;
  a.rows = T.rows.as<int32_t>(), a.row_pair = T.rp.as<int32_t>(), a.n_rows = n_rows, a.stride = pair_stride;
  a.kfs = T.kfs.as<TriNewKf>(), a.keys = S.k.as<vieo_keypoint>(), a.uright = S.u.as<float>(), a.key_cam = S.kc.as<uint8_t>();
  a.nrm = T.nrm.as<double2>(), a.depth = T.depth.as<float>(), a.key_group = T.grp.as<int32_t>();
  a.group_p3d = T.p3d.as<double>(), a.scale = T.scale.as<float>(), a.sigma2 = T.sigma2.as<float>();
  a.th_far_pts = th_far_pts, a.status = T.st.as<int8_t>(), a.x3d = T.x3d.as<double>(), a.x3d_f = T.x3df.as<float>();
  if (rig)
    hipLaunchKernelGGL(k_tri_new_points<8>, dim3((n_rows + 63) / 64), dim3(64), 0, nullptr, a);
  else
    hipLaunchKernelGGL(k_tri_new_points<2>, dim3((n_rows + 63) / 64), dim3(64), 0, nullptr, a);
  VIEO_HIP_CHECK(hipGetLastError());
  std::vector<int8_t> st(n_rows);
  std::vector<double> x3d((size_t)n_rows * 3);
  std::vector<float> x3df((size_t)n_rows * 3);
  VIEO_HIP_CHECK(hipMemcpy(st.data(), T.st.p, n_rows, hipMemcpyDeviceToHost));
  VIEO_HIP_CHECK(hipMemcpy(x3d.data(), T.x3d.p, (size_t)n_rows * 24, hipMemcpyDeviceToHost));
  VIEO_HIP_CHECK(hipMemcpy(x3df.data(), T.x3df.p, (size_t)n_rows * 12, hipMemcpyDeviceToHost));
  for (int r = 0; r < n_rows; r++) {
    const size_t at = row_dst[r];
    h_status[at] = st[r];
    memcpy(h_x3d + at * 3, &x3d[(size_t)r * 3], 24), memcpy(h_x3d_f + at * 3, &x3df[(size_t)r * 3], 12);
    h_n_new[row_pair[r]] += st[r] >= 0;
  }
  return VIEO_OK;
}

}  // namespace vieo

using namespace vieo;

extern "C" int vieo_search_for_triangulation(const vieo_tri_keyframe* kf1, const vieo_tri_keyframe* kf2s, int n_kf2,
                                             int only_stereo, int check_orientation, int32_t pair_capacity,
                                             int32_t pair_stride, int32_t* h_pairs, int32_t* h_n_pairs,
                                             int32_t* h_n_matches) {
  return tri_search_impl(kf1, kf2s, n_kf2, only_stereo, check_orientation, pair_capacity, pair_stride, h_pairs,
                         h_n_pairs, h_n_matches, nullptr, nullptr);
}

extern "C" int vieo_triangulate_new_points(const vieo_tri_keyframe* kf1, const vieo_tri_stereo* st1,
                                           const vieo_tri_keyframe* kf2s, const vieo_tri_stereo* st2s, int n_kf2,
                                           float th_far_pts, int32_t pair_capacity, int32_t pair_stride,
                                           const int32_t* h_pairs, const int32_t* h_n_pairs, int8_t* h_status,
                                           double* h_x3d, float* h_x3d_f, int32_t* h_n_new) {
  if (!kf1 || !st1 || n_kf2 < 0 || pair_capacity < 0) return VIEO_E_INVALID;
  if (n_kf2 == 0) return VIEO_OK;  // a key frame without neighbours
  if (!kf2s || !st2s || !h_n_pairs || !h_n_new || (pair_capacity > 0 && (!h_pairs || !h_status || !h_x3d || !h_x3d_f)))
    return VIEO_E_INVALID;
  std::vector<int> n_groups;
  int rc = tri_new_check(kf1, st1, kf2s, st2s, n_kf2, pair_capacity, pair_stride, n_groups);
  if (rc != VIEO_OK) return rc;
  if ((rc = require_device()) != VIEO_OK) return rc;
  return tri_new_points_impl(kf1, st1, kf2s, st2s, n_kf2, th_far_pts, pair_capacity, pair_stride, h_pairs, h_n_pairs,
                             n_groups, false, h_status, h_x3d, h_x3d_f, h_n_new);
}

extern "C" int vieo_create_new_map_points(const vieo_tri_keyframe* kf1, const vieo_tri_stereo* st1,
                                          const vieo_tri_keyframe* kf2s, const vieo_tri_stereo* st2s, int n_kf2,
                                          int only_stereo, int check_orientation, float th_far_pts,
                                          int32_t pair_capacity, int32_t pair_stride, int32_t* h_pairs,
                                          int32_t* h_n_pairs, int32_t* h_n_matches, int8_t* h_status, double* h_x3d,
                                          float* h_x3d_f, int32_t* h_n_new) {
  if (!kf1 || !st1 || n_kf2 < 0 || pair_capacity < 0) return VIEO_E_INVALID;
  if (n_kf2 == 0) return VIEO_OK;
  if (!kf2s || !st2s || !h_n_pairs || !h_n_matches || !h_n_new ||
      (pair_capacity > 0 && (!h_pairs || !h_status || !h_x3d || !h_x3d_f)))
    return VIEO_E_INVALID;
  std::vector<int> n_groups;
  int rc = tri_new_check(kf1, st1, kf2s, st2s, n_kf2, pair_capacity, pair_stride, n_groups);
  if (rc != VIEO_OK) return rc;
  std::vector<uint8_t> skip(n_kf2);
  for (int p = 0; p < n_kf2; p++) skip[p] = tri_baseline_short(*st1, st2s[p]);
  bool resident = false;
  rc = tri_search_impl(kf1, kf2s, n_kf2, only_stereo, check_orientation, pair_capacity, pair_stride, h_pairs, h_n_pairs,
                       h_n_matches, skip.data(), &resident);
  if (rc != VIEO_OK) return rc;
  return tri_new_points_impl(kf1, st1, kf2s, st2s, n_kf2, th_far_pts, pair_capacity, pair_stride, h_pairs, h_n_pairs,
                             n_groups, resident, h_status, h_x3d, h_x3d_f, h_n_new);
}
