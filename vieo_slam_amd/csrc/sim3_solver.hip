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
// host: the handle
struct vieo_sim3_solver {
  struct Cand {
    int n = 0, n1 = 0, words = 0;
    int min_inliers = 0, max_its = 1;
    bool alive = false;  // N >= mRansacMinInliers
    std::vector<int32_t> index1;
    std::vector<double> sRt;      // [n_rows][13]
    std::vector<int32_t> count;   // [n_rows]
    std::vector<uint64_t> mask;   // [n_rows][words]
    int iterations = 0, best_inliers = 0, best_row = -1;  // Sim3Solver's state between iterate calls
  };
  std::vector<Cand> cands;
  std::vector<int32_t> samples;  // [K][S][3]
  int n_rows = 0;
};

namespace vieo {

// SetRansacParameters (Sim3Solver.cc:118-141) for N >= minInliers
static int sim3_max_iterations(const vieo_sim3_params& P, int N) {
  const float epsilon = (float)P.min_inliers / N;
  int nIterations;
  if (P.min_inliers == N)
    nIterations = 1;
  else {
    const double its = std::ceil(std::log(1 - P.probability) / std::log(1 - std::pow((double)epsilon, 3.0)));
    nIterations = !(its < 2147483647.0) ? 2147483647 : its < 1.0 ? 1 : (int)its;
  }
  return std::max(1, std::min(nIterations, P.max_iterations));
}

struct Sim3Scratch {
  DevBuf cands, x1, x2, me, ci, cams, smp, srt, cnt, mask;
};
static thread_local Sim3Scratch g_sim3;

static int sim3_build(vieo_sim3_solver& H, const vieo_sim3_candidate* cands, int K) {
  const int S = H.n_rows;
  int rc = require_device();
  if (rc != VIEO_OK) return rc;
  std::vector<Sim3CandDev> cd(K);
  std::vector<CamD> cams;
  size_t n_all = 0, words_all = 0;
  for (int c = 0; c < K; c++) {
    vieo_sim3_solver::Cand& Q = H.cands[c];
    cd[c] = Sim3CandDev{(int)n_all, Q.n, Q.alive ? Q.words : 0, (int)words_all, (int)cams.size(),
                        (int)cams.size() + cands[c].n_cams1, cands[c].fix_scale != 0, 0};
    for (int side = 0; side < 2; side++)
      for (int i = 0; i < (side ? cands[c].n_cams2 : cands[c].n_cams1); i++) {
        CamD d;
        cam_from_abi((side ? cands[c].cams2 : cands[c].cams1)[i], d);
        cams.push_back(d);
      }
    n_all += Q.n;
    if (Q.alive) words_all += (size_t)S * Q.words;
  }
  if (words_all == 0) return VIEO_OK;  // no candidate has a solver: nothing to compute
  std::vector<float> x1(3 * n_all), x2(3 * n_all), me(2 * n_all);
  std::vector<int32_t> ci(n_all);
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
  if ((rc = G.cands.ensure(K * sizeof(Sim3CandDev))) != VIEO_OK || (rc = G.x1.ensure(x1.size() * 4)) != VIEO_OK ||
      (rc = G.x2.ensure(x2.size() * 4)) != VIEO_OK || (rc = G.me.ensure(me.size() * 4)) != VIEO_OK ||
      (rc = G.ci.ensure(ci.size() * 4)) != VIEO_OK || (rc = G.cams.ensure(cams.size() * sizeof(CamD))) != VIEO_OK ||
      (rc = G.smp.ensure(jobs * 12)) != VIEO_OK || (rc = G.srt.ensure(jobs * 104)) != VIEO_OK ||
      (rc = G.cnt.ensure(jobs * 4)) != VIEO_OK || (rc = G.mask.ensure(words_all * 8)) != VIEO_OK)
    return rc;
  VIEO_HIP_CHECK(hipMemcpy(G.cands.p, cd.data(), K * sizeof(Sim3CandDev), hipMemcpyHostToDevice));
  VIEO_HIP_CHECK(hipMemcpy(G.x1.p, x1.data(), x1.size() * 4, hipMemcpyHostToDevice));
  VIEO_HIP_CHECK(hipMemcpy(G.x2.p, x2.data(), x2.size() * 4, hipMemcpyHostToDevice));
  VIEO_HIP_CHECK(hipMemcpy(G.me.p, me.data(), me.size() * 4, hipMemcpyHostToDevice));
  VIEO_HIP_CHECK(hipMemcpy(G.ci.p, ci.data(), ci.size() * 4, hipMemcpyHostToDevice));
  VIEO_HIP_CHECK(hipMemcpy(G.cams.p, cams.data(), cams.size() * sizeof(CamD), hipMemcpyHostToDevice));
  VIEO_HIP_CHECK(hipMemcpy(G.smp.p, H.samples.data(), jobs * 12, hipMemcpyHostToDevice));
  VIEO_HIP_CHECK(hipMemset(G.srt.p, 0, jobs * 104));
  VIEO_HIP_CHECK(hipMemset(G.cnt.p, 0, jobs * 4));
  hipLaunchKernelGGL(k_sim3_hypotheses, dim3((unsigned)jobs), dim3(64), 0, nullptr, G.cands.as<Sim3CandDev>(), S,
                     G.x1.as<float>(), G.x2.as<float>(), G.me.as<float>(), G.ci.as<int>(), G.cams.as<CamD>(),
                     G.smp.as<int>(), G.srt.as<double>(), G.cnt.as<int>(), G.mask.as<unsigned long long>());
  VIEO_HIP_CHECK(hipGetLastError());
  std::vector<double> srt(jobs * 13);
  std::vector<int32_t> cnt(jobs);
  std::vector<uint64_t> mask(words_all);
  VIEO_HIP_CHECK(hipMemcpy(srt.data(), G.srt.p, jobs * 104, hipMemcpyDeviceToHost));
  VIEO_HIP_CHECK(hipMemcpy(cnt.data(), G.cnt.p, jobs * 4, hipMemcpyDeviceToHost));
  VIEO_HIP_CHECK(hipMemcpy(mask.data(), G.mask.p, words_all * 8, hipMemcpyDeviceToHost));
  for (int c = 0; c < K; c++) {
    vieo_sim3_solver::Cand& Q = H.cands[c];
    if (!Q.alive) continue;
    Q.sRt.assign(srt.begin() + (size_t)c * S * 13, srt.begin() + (size_t)(c + 1) * S * 13);
    Q.count.assign(cnt.begin() + (size_t)c * S, cnt.begin() + (size_t)(c + 1) * S);
    Q.mask.assign(mask.begin() + cd[c].mask_off, mask.begin() + cd[c].mask_off + (size_t)S * Q.words);
  }
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
  vieo_sim3_solver* H = new vieo_sim3_solver;
  H->n_rows = n_rows;
  H->cands.resize(n_cands);
  H->samples.assign((size_t)n_cands * n_rows * 3, 0);
  for (int c = 0; c < n_cands; c++) {
    vieo_sim3_solver::Cand& Q = H->cands[c];
    Q.n = cands[c].n, Q.n1 = cands[c].n1, Q.words = (Q.n + 63) / 64;
    Q.index1.assign(cands[c].index1, cands[c].index1 + Q.n);
    Q.min_inliers = params->min_inliers;
    Q.alive = Q.n >= Q.min_inliers;  // (min_inliers >= 3: a solver has its 3 points)
    if (!Q.alive) continue;
    Q.max_its = sim3_max_iterations(*params, Q.n);
    int32_t* dst = &H->samples[(size_t)c * n_rows * 3];
    for (int r = 0; r < n_rows; r++) {
      if (!samples) {
        pnp_draw(seed, c, r, Q.n, 3, dst + 3 * r);  // the generator of pnp.hip, swap-with-back as :164-178
        continue;
      }
      const int32_t* src = samples + ((size_t)c * n_rows + r) * 3;
      for (int i = 0; i < 3; i++) {
        bool ok = src[i] >= 0 && src[i] < Q.n;
        for (int j = 0; ok && j < i; j++) ok = src[j] != src[i];
        if (!ok) {
          set_error("Sim3Solver: candidate %d, sample row %d: index %d out of range or drawn twice", c, r, src[i]);
          delete H;
          return VIEO_E_INVALID;
        }
        dst[3 * r + i] = src[i];
      }
    }
  }
  const int rc = sim3_build(*H, cands, n_cands);
  if (rc != VIEO_OK) {
    delete H;
    return rc;
  }
  *out = H;
  return VIEO_OK;
}

void vieo_sim3_destroy(vieo_sim3_solver* h) { delete h; }

int vieo_sim3_get_info(const vieo_sim3_solver* h, int cand, vieo_sim3_info* info) {
  if (!h || !info || cand < 0 || cand >= (int)h->cands.size()) return VIEO_E_INVALID;
  const vieo_sim3_solver::Cand& Q = h->cands[cand];
  info->n = Q.n, info->n1 = Q.n1, info->min_inliers = Q.min_inliers, info->max_its = Q.max_its;
  info->n_rows = h->n_rows, info->mask_words = Q.words;
  info->iterations = Q.iterations, info->best_inliers = Q.best_inliers, info->best_row = Q.best_row, info->reserved = 0;
  return VIEO_OK;
}

int vieo_sim3_iterate(vieo_sim3_solver* h, int cand, int n_iterations, int32_t* found, float* T12, uint8_t* inliers,
                      int32_t* n_inliers, int32_t* no_more, int32_t* row_used) {
  using namespace vieo;
  if (!h || cand < 0 || cand >= (int)h->cands.size() || !found || !T12 || !n_inliers || !no_more) return VIEO_E_INVALID;
  vieo_sim3_solver::Cand& Q = h->cands[cand];
  if (Q.n1 > 0 && !inliers) return VIEO_E_INVALID;
  *found = 0, *n_inliers = 0, *no_more = 0;
  if (row_used) *row_used = -1;
  if (Q.n1 > 0) memset(inliers, 0, Q.n1);  // vbInliers = vector<bool>(mN1, false)
  if (!Q.alive) {  // N < mRansacMinInliers
    *no_more = 1;
    return VIEO_OK;
  }
  int current = 0;
  while (Q.iterations < Q.max_its && current < n_iterations) {
    if (Q.iterations >= h->n_rows) {
      set_error("Sim3Solver: candidate %d needs sample row %d, the table has %d", cand, Q.iterations, h->n_rows);
      return VIEO_E_CAPACITY;
    }
    const int row = Q.iterations;
    current++, Q.iterations++;
    if (Q.count[row] < Q.best_inliers) continue;
    Q.best_inliers = Q.count[row], Q.best_row = row;
    if (Q.count[row] > Q.min_inliers) {
      const double* o = &Q.sRt[(size_t)row * 13];
      for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) T12[4 * r + c] = (float)(o[12] * o[3 * r + c]);
        T12[4 * r + 3] = (float)o[9 + r];
      }
      T12[12] = T12[13] = T12[14] = 0.f, T12[15] = 1.f;
      const uint64_t* m = &Q.mask[(size_t)row * Q.words];
      for (int i = 0; i < Q.n; i++)
        if ((m[i / 64] >> (i % 64)) & 1) inliers[Q.index1[i]] = 1;
      *found = 1, *n_inliers = Q.count[row];
      if (row_used) *row_used = row;
      return VIEO_OK;
    }
  }
  if (Q.iterations >= Q.max_its) *no_more = 1;
  return VIEO_OK;
}

int vieo_sim3_get_estimate(const vieo_sim3_solver* h, int cand, float* R12, float* t12, float* s12) {
  if (!h || cand < 0 || cand >= (int)h->cands.size() || !R12 || !t12 || !s12) return VIEO_E_INVALID;
  const vieo_sim3_solver::Cand& Q = h->cands[cand];
  if (Q.best_row < 0) {
    vieo::set_error("Sim3Solver: candidate %d has no estimate yet", cand);
    return VIEO_E_EMPTY;
  }
  const double* o = &Q.sRt[(size_t)Q.best_row * 13];
  for (int i = 0; i < 9; i++) R12[i] = (float)o[i];
  for (int i = 0; i < 3; i++) t12[i] = (float)o[9 + i];
  *s12 = (float)o[12];
  return VIEO_OK;
}

int vieo_sim3_tap_rows(const vieo_sim3_solver* h, int cand, int32_t* samples, double* sRt, int32_t* count, uint64_t* mask) {
  if (!h || cand < 0 || cand >= (int)h->cands.size()) return VIEO_E_INVALID;
  const vieo_sim3_solver::Cand& Q = h->cands[cand];
  const size_t S = h->n_rows;
  if (samples) memcpy(samples, &h->samples[(size_t)cand * S * 3], S * 12);
  if (!Q.alive) {
    if (sRt) memset(sRt, 0, S * 104);
    if (count) memset(count, 0, S * 4);
    if (mask) memset(mask, 0, S * Q.words * 8);
    return VIEO_OK;
  }
  if (sRt) memcpy(sRt, Q.sRt.data(), S * 104);
  if (count) memcpy(count, Q.count.data(), S * 4);
  if (mask) memcpy(mask, Q.mask.data(), S * Q.words * 8);
  return VIEO_OK;
}

}  // extern "C"
