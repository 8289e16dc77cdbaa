// sim3_solver.hip -- Sim3Solver for a batch of loop candidates (reference src/Sim3Solver.cc, include/Sim3Solver.h;
// LoopClosing::ComputeSim3, LoopClosing.cc:308-489).
//   k_sim3_hypotheses  every row of the sample table of every candidate: ComputeSim3 (Horn's closed form) on the row's
//                      3 pairs, then CheckInliers over the candidate's n correspondences
//   host               vieo_sim3_iterate replays Sim3Solver::iterate over the table (look-ups only)
// Mapping: one wavefront per row.  A row's work is its n-long inlier check (four projections per correspondence); Horn's
// form is a few hundred dependent FP64 operations on wave-uniform inputs, so every lane computes it redundantly (no
// cross-lane traffic, no LDS, and its branches are wave-uniform).  Lane i then checks correspondence 64 w + i: the
// reads of X1 / X2 / max_err are consecutive across the lanes, __ballot of the test is mask word w as it is stored,
// and its popcount accumulates the count: no atomics.  The 4 x 4 eigen-solver is a cyclic Jacobi in a fixed pair order
// (reproducible run to run).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "common.h"
#include "sim3_solver_device.h"

namespace vieo {

// block = candidate * n_rows + row; a candidate without a solver (n below mRansacMinInliers: iterate never looks at
// its rows) has words == 0
__global__ void __launch_bounds__(64)
k_sim3_hypotheses(const Sim3CandDev* __restrict__ cands, int n_rows, const float* __restrict__ X1,
                  const float* __restrict__ X2, const float* __restrict__ max_err, const int* __restrict__ cam_idx,
                  const CamD* __restrict__ cams, const int* __restrict__ samples, double* __restrict__ sRt,
                  int* __restrict__ count, unsigned long long* __restrict__ mask) {
  const int job = blockIdx.x, lane = threadIdx.x;
  const Sim3CandDev C = cands[job / n_rows];
  if (C.words == 0) return;
  const int row = job % n_rows;
  const float* x1 = X1 + 3 * (size_t)C.off;
  const float* x2 = X2 + 3 * (size_t)C.off;
  double P1[3][3], P2[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int g = samples[3 * (size_t)job + i];
#pragma unroll
    for (int c = 0; c < 3; ++c) P1[i][c] = (double)x1[3 * g + c], P2[i][c] = (double)x2[3 * g + c];
  }
  double R[3][3], t[3], s;
  s3s_horn(P1, P2, C.fix_scale != 0, R, t, s);
  if (lane == 0) {
    double* o = sRt + 13 * (size_t)job;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) o[3 * r + c] = R[r][c];
      o[9 + r] = t[r];
    }
    o[12] = s;
  }
  Sim3Pose T;
  s3s_pose(R, t, s, T);
  int cnt = 0;
  for (int w = 0; w < C.words; ++w) {
    const int i = 64 * w + lane;
    bool ok = false;
    if (i < C.n) {
      const size_t g = (size_t)C.off + i;
      const int ci = cam_idx[g];
      ok = s3s_is_inlier(T, cams[C.cam_off1 + (ci & 0xFFFF)], cams[C.cam_off2 + (ci >> 16)], X1 + 3 * g, X2 + 3 * g,
                         max_err[2 * g], max_err[2 * g + 1]);
    }
    const unsigned long long bits = __ballot(ok);
    if (lane == 0) mask[C.mask_off + (size_t)row * C.words + w] = bits;
    cnt += __popcll(bits);
  }
  if (lane == 0) count[job] = cnt;
}

}  // namespace vieo

// ------------------------------------------------------------------------------------------------------------------
// host: the handle vieo_sim3_solver (its table and the replay of iterate: ransac_table.h), staging and the launch
#include <memory>

#include "ransac_table.h"

namespace vieo {

struct Sim3Scratch {
  DevBuf cands, x1, x2, me, ci, cams, smp, srt, cnt, mask;
};
static thread_local Sim3Scratch g_sim3;

static int sim3_build(vieo_sim3_solver& H, const vieo_sim3_candidate* cands, int K) {
  const int S = H.n_rows;
  int rc = require_device();
  if (rc != VIEO_OK) return rc;
  const RansacLayout L = H.layout();
  std::vector<Sim3CandDev> cd(K);
  std::vector<CamD> cams;
  for (int c = 0; c < K; c++) {
    cd[c] = Sim3CandDev{L.off[c], H.cands[c].n, L.words[c], L.mask_off[c], (int)cams.size(),
                        (int)cams.size() + cands[c].n_cams1, cands[c].fix_scale != 0, 0};
    for (int side = 0; side < 2; side++)
      for (int i = 0; i < (side ? cands[c].n_cams2 : cands[c].n_cams1); i++) {
        CamD d;
        cam_from_abi((side ? cands[c].cams2 : cands[c].cams1)[i], d);
        cams.push_back(d);
      }
  }
  if (L.words_all == 0) return VIEO_OK;  // no candidate has a solver: nothing to compute
  std::vector<float> x1(3 * L.n_all), x2(3 * L.n_all), me(2 * L.n_all);
  std::vector<int32_t> ci(L.n_all);
  for (int c = 0; c < K; c++) {
    const size_t off = cd[c].off, n = cd[c].n;
    if (!n) continue;
    memcpy(&x1[3 * off], cands[c].X1, n * 12), memcpy(&x2[3 * off], cands[c].X2, n * 12);
    for (size_t i = 0; i < n; i++) {
      me[2 * (off + i)] = (float)cands[c].max_err1[i], me[2 * (off + i) + 1] = (float)cands[c].max_err2[i];
      ci[off + i] = cands[c].cam1[i] | (cands[c].cam2[i] << 16);
    }
  }
  Sim3Scratch& G = g_sim3;
  const size_t jobs = (size_t)K * S;
  if ((rc = dev_put(G.cands, cd.data(), K * sizeof(Sim3CandDev))) != VIEO_OK || (rc = dev_put(G.x1, x1.data(), x1.size() * 4)) != VIEO_OK ||
      (rc = dev_put(G.x2, x2.data(), x2.size() * 4)) != VIEO_OK || (rc = dev_put(G.me, me.data(), me.size() * 4)) != VIEO_OK ||
      (rc = dev_put(G.ci, ci.data(), ci.size() * 4)) != VIEO_OK || (rc = dev_put(G.cams, cams.data(), cams.size() * sizeof(CamD))) != VIEO_OK ||
      (rc = dev_put(G.smp, H.samples.data(), jobs * 12)) != VIEO_OK || (rc = dev_zero(G.srt, jobs * 104)) != VIEO_OK ||
      (rc = dev_zero(G.cnt, jobs * 4)) != VIEO_OK || (rc = G.mask.ensure(L.words_all * 8)) != VIEO_OK)
    return rc;
  hipLaunchKernelGGL(k_sim3_hypotheses, dim3((unsigned)jobs), dim3(64), 0, nullptr, G.cands.as<Sim3CandDev>(), S,
                     G.x1.as<float>(), G.x2.as<float>(), G.me.as<float>(), G.ci.as<int>(), G.cams.as<CamD>(),
                     G.smp.as<int>(), G.srt.as<double>(), G.cnt.as<int>(), G.mask.as<unsigned long long>());
  VIEO_HIP_CHECK(hipGetLastError());
  std::vector<double> srt(jobs * 13);
  std::vector<int32_t> cnt(jobs);
  std::vector<uint64_t> mask(L.words_all);
  if ((rc = dev_get(srt.data(), G.srt, jobs * 104)) != VIEO_OK || (rc = dev_get(cnt.data(), G.cnt, jobs * 4)) != VIEO_OK ||
      (rc = dev_get(mask.data(), G.mask, L.words_all * 8)) != VIEO_OK)
    return rc;
  for (int c = 0; c < K; c++)
    if (H.cands[c].alive) H.cands[c].slice(c, S, L.mask_off[c], srt.data(), cnt.data(), mask.data());
  return VIEO_OK;
}

}  // namespace vieo

extern "C" {

int vieo_sim3_create(vieo_sim3_solver** out, const vieo_sim3_candidate* cands, int n_cands, const vieo_sim3_params* params,
                     const int32_t* samples, int n_rows, uint64_t seed) {
  using namespace vieo;
  if (!out) return VIEO_E_INVALID;
  *out = nullptr;
  if (!cands || n_cands <= 0 || !params) {
    set_error("Sim3Solver: null argument or no candidate");
    return VIEO_E_INVALID;
  }
  if (n_rows <= 0 || n_rows > kSim3MaxRows) {
    set_error("Sim3Solver: %d sample rows, 1 ... %d are possible", n_rows, kSim3MaxRows);
    return VIEO_E_INVALID;
  }
  if (!(params->probability > 0 && params->probability < 1) || params->max_iterations < 1 || params->min_inliers < 3) {
    set_error("Sim3Solver: RANSAC parameters out of range (the minimal set is 3 points)");
    return VIEO_E_INVALID;
  }
  for (int c = 0; c < n_cands; c++) {
    const vieo_sim3_candidate& C = cands[c];
    if (C.n < 0 || C.n1 < 0 || C.n_cams1 < 1 || C.n_cams1 > kSim3MaxCams || C.n_cams2 < 1 || C.n_cams2 > kSim3MaxCams ||
        !C.cams1 || !C.cams2 ||
        (C.n > 0 && (!C.X1 || !C.X2 || !C.max_err1 || !C.max_err2 || !C.index1 || !C.cam1 || !C.cam2))) {
      set_error("Sim3Solver: candidate %d is inconsistent", c);
      return VIEO_E_INVALID;
    }
    CamD d;
    for (int i = 0; i < C.n_cams1 + C.n_cams2; i++)
      if (!cam_from_abi(i < C.n_cams1 ? C.cams1[i] : C.cams2[i - C.n_cams1], d)) {
        set_error("Sim3Solver: candidate %d, unknown camera model", c);
        return VIEO_E_INVALID;
      }
    for (int i = 0; i < C.n; i++)
      if (C.index1[i] < 0 || C.index1[i] >= C.n1 || C.cam1[i] < 0 || C.cam1[i] >= C.n_cams1 || C.cam2[i] < 0 ||
          C.cam2[i] >= C.n_cams2 || C.max_err1[i] < 0 || C.max_err2[i] < 0) {
        set_error("Sim3Solver: candidate %d, correspondence %d: index1 %d of %d, cameras %d of %d / %d of %d, or a negative "
                  "threshold", c, i, C.index1[i], C.n1, C.cam1[i], C.n_cams1, C.cam2[i], C.n_cams2);
        return VIEO_E_INVALID;
      }
  }
  std::unique_ptr<vieo_sim3_solver> H(new vieo_sim3_solver);
  H->n_rows = n_rows;
  H->cands.resize(n_cands);
  for (int c = 0; c < n_cands; c++) {
    H->cands[c].set(cands[c].n, cands[c].n1, cands[c].index1);
    sim3_set_ransac_parameters(H->cands[c], *params);
  }
  RansacBadSample bad;
  if (!H->fill_samples(samples, seed, bad)) {
    set_error("Sim3Solver: candidate %d, sample row %d: index %d out of range or drawn twice", bad.cand, bad.row, bad.index);
    return VIEO_E_INVALID;
  }
  const int rc = sim3_build(*H, cands, n_cands);
  if (rc == VIEO_OK) *out = H.release();
  return rc;
}

void vieo_sim3_destroy(vieo_sim3_solver* h) { delete h; }

int vieo_sim3_get_info(const vieo_sim3_solver* h, int cand, vieo_sim3_info* info) {
  if (!h || !info || !h->has(cand)) return VIEO_E_INVALID;
  const vieo::Sim3Cand& Q = h->cands[cand];
  info->n = Q.n, info->n1 = Q.n_out, info->min_inliers = Q.min_inliers, info->max_its = Q.max_its;
  info->n_rows = h->n_rows, info->mask_words = Q.words;
  info->iterations = Q.iterations, info->best_inliers = Q.best_inliers, info->best_row = Q.best_row, info->reserved = 0;
  return VIEO_OK;
}

int vieo_sim3_iterate(vieo_sim3_solver* h, int cand, int n_iterations, int32_t* found, float* T12, uint8_t* inliers,
                      int32_t* n_inliers, int32_t* no_more, int32_t* row_used) {
  if (!h || !h->has(cand) || !found || !T12 || !n_inliers || !no_more || (h->cands[cand].n_out > 0 && !inliers)) return VIEO_E_INVALID;
  return vieo::sim3_iterate(*h, cand, n_iterations, found, T12, inliers, n_inliers, no_more, row_used);
}

int vieo_sim3_get_estimate(const vieo_sim3_solver* h, int cand, float* R12, float* t12, float* s12) {
  if (!h || !h->has(cand) || !R12 || !t12 || !s12) return VIEO_E_INVALID;
  return vieo::sim3_get_estimate(*h, cand, R12, t12, s12);
}

int vieo_sim3_tap_rows(const vieo_sim3_solver* h, int cand, int32_t* samples, double* sRt, int32_t* count, uint64_t* mask) {
  return h && h->has(cand) ? h->tap_rows(cand, samples, sRt, count, mask) : VIEO_E_INVALID;
}

}  // extern "C"
