// sim3_optimize.hip -- Optimizer::OptimizeSim3 (reference src/Optimizer.cc:2689-2918) for a list of loop visits in one
// call (vieo_optimize_sim3).  Host: the correspondences of every visit (one record each: both camera-frame points, both
// observations, both informations, both cameras), one copy up.  Device: k_sim3_optimize, one wavefront per visit, runs the
// whole visit -- optimize(5), the first check, optimize(5 | 10), the second check -- without a host round trip: the lanes
// stride over the correspondences, every lane keeps its part of H (28), b (7) and the robust chi2 in FP64 registers,
// wave_sum_f64 (DPP, fixed tree) makes the sums uniform, the 7 x 7 LDL^T, the retraction and the policy run uniformly on
// every lane.  The chi2 of the latest error pass sits in a per-visit buffer: a check reads it as the last lambda trial left
// it, accepted or not, which is what g2o's edges hold after pop().  An erased correspondence is a flag, not a compaction.
// A fixed lane <-> correspondence map and the fixed tree make a visit's result independent of its neighbours and of the run.
// One copy back, one synchronisation.  The lane functions are sim3_optimize_device.h's.
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "common.h"
#include "sim3_optimize_device.h"
#include "wave_ops.h"

namespace vieo {
namespace {

const int kOptMaxKeys = 8192, kOptMaxCams = 4, kOptMaxVisits = 16384;  // the limits of vieo_search_by_sim3

struct WaveLanes {
  int lane;
  __device__ __forceinline__ bool leader() const { return lane == 0; }
  template <int N, class F>
  __device__ __forceinline__ void run(F f, double* out) {
    double part[N];
    f(lane, 64, part);
#pragma unroll
    for (int i = 0; i < N; i++) out[i] = wave_sum_f64(part[i]);
  }
};

__global__ __launch_bounds__(64) void k_sim3_optimize(const S3oVisit* __restrict__ visits, const S3oCorr* __restrict__ corr,
                                                      const CamD* __restrict__ cams, double* __restrict__ chi,
                                                      double* __restrict__ chi_check, int32_t* __restrict__ erased,
                                                      double* __restrict__ trace, S3oOut* __restrict__ out) {
  const int v = blockIdx.x, lane = threadIdx.x;
  const S3oVisit P = visits[v];
  if (P.n <= 0) return;  // (uniform)
  S3oView V;
  V.corr = corr + P.first, V.cams = cams, V.n = P.n;
  V.chi = chi + 2 * (size_t)P.first, V.chi_check = chi_check + 4 * (size_t)P.first, V.erased = erased + P.first;
  V.trace = trace + (size_t)v * S3O_MAX_TRIALS * 4;
  for (int k = lane; k < P.n; k += 64) {
    V.erased[k] = 0;
    V.chi_check[2 * k] = V.chi_check[2 * k + 1] = 0;
    V.chi_check[2 * (P.n + k)] = V.chi_check[2 * (P.n + k) + 1] = 0;
  }
  WaveLanes L{lane};
  S3oOut O;
  s3o_visit(L, V, P, O);
  if (lane == 0) out[v] = O;
}

// a key frame of the call as the host reads it
struct OptKfHost {
  const vieo_loop_keyframe* K = nullptr;
  int n = 0;
  std::vector<std::pair<int, int>> by_id;  // (mp_id, key) ascending: GetIndexInKeyFrame
  int cam(int i) const { return K->cam_of_key ? K->cam_of_key[i] : 0; }
  int first_key_of(int id) const {  // *GetIndexInKeyFrame(pKF2).begin()
    auto lo = std::lower_bound(by_id.begin(), by_id.end(), std::make_pair(id, INT_MIN));
    return lo != by_id.end() && lo->first == id ? lo->second : -1;
  }
};

// the grounds on which vieo_search_by_sim3 refuses a key frame
int opt_kf_prepare(const vieo_loop_keyframe* K, const vieo_loop_keyframe* first, const char* who, int slot, OptKfHost& H, CamD* cams) {
  const int n = K->bow.n_keys;
  if (n < 0 || (n > 0 && (!K->bow.keys || !K->bow.descriptors || !K->bow.mp_id || !K->points)) || !K->cams) {
    set_error("%s: key frame %d has a null pointer or a negative key count", who, slot);
    return VIEO_E_INVALID;
  }
  if (n > kOptMaxKeys) {
    set_error("%s: key frame %d has %d keys (limit %d)", who, slot, n, kOptMaxKeys);
    return VIEO_E_CAPACITY;
  }
  if (K->n_cams < 1 || K->n_cams > kOptMaxCams || K->n_levels < 1 || K->n_levels > 16) {
    set_error("%s: key frame %d has n_cams = %d (1..4), n_levels = %d (1..16)", who, slot, K->n_cams, K->n_levels);
    return VIEO_E_INVALID;
  }
  if (K->n_cams != first->n_cams || memcmp(K->bounds, first->bounds, sizeof(float) * 4 * K->n_cams) != 0) {
    set_error("%s: key frame %d differs from the current key frame in n_cams or in the image bounds", who, slot);
    return VIEO_E_INVALID;
  }
  for (int c = 0; c < K->n_cams; ++c) {
    CamD& d = cams[c];
    if (!cam_from_abi(K->cams[c], d)) {
      set_error("%s: camera %d of key frame %d has an unknown model or coefficient count", who, c, slot);
      return VIEO_E_INVALID;
    }
    const float* T = K->Tcr[c];  // SetParams(cam): Rcb = GetTcr().rotationMatrix(), tcb = GetTcr().translation()
    for (int r = 0; r < 3; ++r) {
      for (int q = 0; q < 3; ++q) d.Rcb[3 * r + q] = (double)T[4 * r + q];
      d.tcb[r] = (double)T[4 * r + 3];
    }
  }
  H.K = K, H.n = n;
  H.by_id.clear();
  for (int i = 0; i < n; ++i) {
    const int c = H.cam(i), o = K->bow.keys[i].octave;
    if (c < 0 || c >= K->n_cams || o < 0 || o >= K->n_levels) {
      set_error("%s: key %d of key frame %d has camera %d (of %d) / octave %d (of %d)", who, i, slot, c, K->n_cams, o, K->n_levels);
      return VIEO_E_INVALID;
    }
    if (K->bow.mp_id[i] >= 0) H.by_id.emplace_back(K->bow.mp_id[i], i);
  }
  std::sort(H.by_id.begin(), H.by_id.end());
  return VIEO_OK;
}

// Vector3f P3Dc = Rcw * Xw + tcw, widened
inline void cam_frame_point(const vieo_loop_keyframe& K, const float* Xw, double* out) {
  for (int r = 0; r < 3; ++r) {
    const float a = (K.Rcw[3 * r] * Xw[0] + K.Rcw[3 * r + 1] * Xw[1]) + K.Rcw[3 * r + 2] * Xw[2];
    out[r] = (double)(a + K.tcw[r]);
  }
}

struct OptTap {
  bool valid = false;
  std::vector<S3oVisit> visits;
  std::vector<S3oOut> out;
  std::vector<int32_t> i1;
  std::vector<double> trace, chi_check;
};
thread_local OptTap g_opt_tap;

}  // namespace
}  // namespace vieo

using namespace vieo;

extern "C" {

int vieo_optimize_sim3(const vieo_loop_keyframe* kf1, const vieo_loop_keyframe* kf2s, int n_kf2, vieo_sim3_opt_visit* visits,
                       int n_visits, float th2, int fix_scale) {
  static const char* who = "OptimizeSim3";
  if (!kf1 || !kf2s || n_kf2 <= 0 || n_visits < 0 || (n_visits > 0 && !visits) || !(th2 > 0.f) || !std::isfinite(th2)) {
    set_error("%s: a null pointer, no candidate, a negative visit count or th2 not positive and finite", who);
    return VIEO_E_INVALID;
  }
  if (n_visits > kOptMaxVisits) {
    set_error("%s: %d visits in one call (limit %d)", who, n_visits, kOptMaxVisits);
    return VIEO_E_CAPACITY;
  }
  const int n_slots = 1 + n_kf2;
  std::vector<OptKfHost> H(n_slots);
  std::vector<CamD> cams((size_t)n_slots * kOptMaxCams + 1);
  int rc;
  for (int f = 0; f < n_slots; ++f)
    if ((rc = opt_kf_prepare(f ? kf2s + (f - 1) : kf1, kf1, who, f, H[f], &cams[(size_t)f * kOptMaxCams])) != VIEO_OK) return rc;
  // usedistort_ false: BOTH edges take a PinholeCamera made from kf1's camera 0 (Optimizer.cc:2752-2756)
  const bool distort = kf1->use_distort != 0;
  const int rect_cam = n_slots * kOptMaxCams;
  cams[rect_cam] = cams[0];
  cams[rect_cam].model = VIEO_CAM_PINHOLE, cams[rect_cam].num_k = 0;
  const int N1 = H[0].n;
  for (int v = 0; v < n_visits; ++v) {
    const vieo_sim3_opt_visit& V = visits[v];
    bool finite = std::isfinite(V.s12);
    for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(V.R12[i]);
    for (int i = 0; i < 3; ++i) finite = finite && std::isfinite(V.t12[i]);
    if (V.kf2 < 0 || V.kf2 >= n_kf2 || (N1 > 0 && !V.match12) || !finite || !(V.s12 > 0)) {
      set_error("%s: visit %d names candidate %d (of %d), has no match12, or an S12 that is not finite with s12 > 0", who, v, V.kf2, n_kf2);
      return VIEO_E_INVALID;
    }
    const int N2 = H[1 + V.kf2].n;
    for (int i = 0; i < N1; ++i)
      if (V.match12[i] < -1 || V.match12[i] >= N2) {
        set_error("%s: match12[%d] = %d of visit %d is outside the candidate's %d keys", who, i, V.match12[i], v, N2);
        return VIEO_E_INVALID;
      }
  }
  if ((rc = require_device()) != VIEO_OK) return rc;
  OptTap& T = g_opt_tap;
  T.valid = false;
  if (n_visits == 0) return VIEO_OK;

  // ---- the correspondences (Optimizer.cc:2757-2850)
  const float delta_f = std::sqrt(th2);  // const float deltaHuber = sqrt(th2)
  std::vector<S3oVisit> P(n_visits);
  std::vector<S3oCorr> corr;
  for (int v = 0; v < n_visits; ++v) {
    const vieo_sim3_opt_visit& V = visits[v];
    const OptKfHost &h1 = H[0], &h2 = H[1 + V.kf2];
    const vieo_loop_keyframe &K1 = *h1.K, &K2 = *h2.K;
    S3oVisit& Q = P[v];
    memset(&Q, 0, sizeof(Q));
    s3o_state_from_sim3(V.R12, V.t12, V.s12, Q.st);
    Q.th2 = (double)th2, Q.delta = (double)delta_f, Q.dsqr = Q.delta * Q.delta;
    Q.first = (int)corr.size(), Q.fix_scale = fix_scale != 0;
    for (int i = 0; i < N1; ++i) {
      const int m = V.match12[i];
      if (m < 0 || K2.bow.mp_id[m] < 0 || K1.bow.mp_id[i] < 0) continue;  // !vpMatches1[i], !pMP1
      const int i2 = h2.first_key_of(K2.bow.mp_id[m]);
      S3oCorr C;
      memset(&C, 0, sizeof(C));
      cam_frame_point(K1, K1.points[i].Xw, C.X1);
      cam_frame_point(K2, K2.points[m].Xw, C.X2);
      const vieo_keypoint &k1 = K1.bow.keys[i], &k2 = K2.bow.keys[i2];
      C.obs1[0] = (double)k1.x, C.obs1[1] = (double)k1.y, C.obs2[0] = (double)k2.x, C.obs2[1] = (double)k2.y;
      C.info1 = (double)K1.inv_level_sigma2[k1.octave], C.info2 = (double)K2.inv_level_sigma2[k2.octave];
      C.cam1 = distort ? h1.cam(i) : rect_cam;
      C.cam2 = distort ? (1 + V.kf2) * kOptMaxCams + h2.cam(i2) : rect_cam;
      C.i1 = i, C.i2 = i2;
      corr.push_back(C);
    }
    Q.n = (int)corr.size() - Q.first;
  }
  const size_t n_corr = corr.size();
  if (n_corr == 0) {
    for (int v = 0; v < n_visits; ++v) {
      vieo_sim3_opt_visit& V = visits[v];
      V.n_inliers = V.n_correspondences = V.n_bad = 0;
      V.iterations[0] = V.iterations[1] = V.trials[0] = V.trials[1] = 0;
    }
    return VIEO_OK;
  }

  // ---- one copy up, one launch, one copy back, one synchronisation
  static thread_local Staging S;
  S.reset();
  const size_t o_vis = S.in(P.data(), P.size() * sizeof(S3oVisit));
  const size_t o_corr = S.in(corr.data(), n_corr * sizeof(S3oCorr));
  const size_t o_cams = S.in(cams.data(), cams.size() * sizeof(CamD));
  const size_t o_out = S.out((size_t)n_visits * sizeof(S3oOut));
  const size_t o_erased = S.out(n_corr * sizeof(int32_t));
  const size_t o_check = S.out(n_corr * 4 * sizeof(double));
  const size_t o_trace = S.out((size_t)n_visits * S3O_MAX_TRIALS * 4 * sizeof(double));
  const size_t o_chi = S.out(n_corr * 2 * sizeof(double));  // working buffer: not copied back
  const size_t back_end = o_chi;
  if ((rc = S.upload(0)) != VIEO_OK) return rc;
  hipLaunchKernelGGL(k_sim3_optimize, dim3((unsigned)n_visits), dim3(64), 0, 0, S.d<S3oVisit>(o_vis), S.d<S3oCorr>(o_corr),
                     S.d<CamD>(o_cams), S.d<double>(o_chi), S.d<double>(o_check), S.d<int32_t>(o_erased), S.d<double>(o_trace),
                     S.d<S3oOut>(o_out));
  VIEO_HIP_CHECK(hipGetLastError());
  VIEO_HIP_CHECK(hipMemcpyAsync((uint8_t*)S.pin.p + o_out, (uint8_t*)S.dev.p + o_out, back_end - o_out, hipMemcpyDeviceToHost, 0));
  VIEO_HIP_CHECK(hipStreamSynchronize(0));

  const S3oOut* out = (const S3oOut*)S.h(o_out);
  const int32_t* erased = (const int32_t*)S.h(o_erased);
  T.visits = P;
  T.out.assign(out, out + n_visits);
  T.i1.resize(n_corr);
  for (size_t k = 0; k < n_corr; ++k) T.i1[k] = corr[k].i1;
  T.chi_check.assign((const double*)S.h(o_check), (const double*)S.h(o_check) + n_corr * 4);
  T.trace.assign((const double*)S.h(o_trace), (const double*)S.h(o_trace) + (size_t)n_visits * S3O_MAX_TRIALS * 4);
  for (int v = 0; v < n_visits; ++v) {
    vieo_sim3_opt_visit& V = visits[v];
    const S3oVisit& Q = P[v];
    if (Q.n == 0) {  // no correspondence: 0, nothing of the visit is touched but the counters
      T.out[v] = S3oOut();
      V.n_inliers = V.n_correspondences = V.n_bad = 0;
      V.iterations[0] = V.iterations[1] = V.trials[0] = V.trials[1] = 0;
      continue;
    }
    const S3oOut& O = out[v];
    for (int k = 0; k < Q.n; ++k)
      if (erased[Q.first + k]) V.match12[corr[Q.first + k].i1] = -1;
    if (!O.returned0) s3o_state_to_sim3(O.st, V.R12, V.t12, &V.s12);
    V.n_inliers = O.returned0 ? 0 : O.n_inliers;
    V.n_correspondences = Q.n, V.n_bad = O.n_bad;
    for (int q = 0; q < 2; ++q) V.iterations[q] = O.iterations[q], V.trials[q] = O.trials[q];
  }
  T.valid = true;
  return VIEO_OK;
}

int vieo_optimize_sim3_trace(int visit, int32_t* n_trials, double* trials, int32_t* n_corr, int32_t* corr_i1, double* chi2) {
  const OptTap& T = g_opt_tap;
  if (!T.valid) return VIEO_E_EMPTY;
  if (visit < 0 || visit >= (int)T.visits.size()) return VIEO_E_INVALID;
  const S3oVisit& Q = T.visits[visit];
  const int nt = std::min<int>(T.out[visit].n_trials, S3O_MAX_TRIALS);
  if (n_trials) *n_trials = nt;
  if (trials && nt) memcpy(trials, T.trace.data() + (size_t)visit * S3O_MAX_TRIALS * 4, (size_t)nt * 4 * sizeof(double));
  if (n_corr) *n_corr = Q.n;
  if (corr_i1 && Q.n) memcpy(corr_i1, T.i1.data() + Q.first, (size_t)Q.n * sizeof(int32_t));
  if (chi2 && Q.n) memcpy(chi2, T.chi_check.data() + 4 * (size_t)Q.first, (size_t)Q.n * 4 * sizeof(double));
  return VIEO_OK;
}

}  // extern "C"
