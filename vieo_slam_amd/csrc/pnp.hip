// pnp.hip -- PnPsolver for a batch of relocalisation candidates (reference src/PnPsolver.cc, include/PnPsolver.h;
// Tracking::Relocalization, Tracking.cc:2567-2604): the rectified configuration (one pinhole K, mvKeysUn) and, as a
// second instance of each kernel, Frame::usedistort_ (the mvKeys of a 1- to 4-camera rig, Pinhole / Radtan / KB8).
//   k_pnp_usun        rig only, once per handle: usun of every correspondence (add_correspondence, :349-358)
//   k_pnp_hypotheses  pass A: every row of the sample table of every candidate -- EPnP on the row's 4 correspondences
//                     (compute_pose and all it calls), then CheckInliers over the candidate's n correspondences
//   host              which rows raise the best-so-far inlier set (the "records": count >= mRansacMinInliers and
//                     strictly greater than every earlier one)
//   k_pnp_refine      pass B: Refine of every record -- EPnP over the record's inliers (M is never stored: its rows
//                     are accumulated into MtM), then CheckInliers
//   host              vieo_pnp_iterate replays PnPsolver::iterate over the two tables (look-ups only)
// Mapping: one hypothesis per lane, 16 per workgroup.  The 12 x 12 MtM and its eigenvectors (2.3 KB per hypothesis)
// live in LDS as [element][lane], so run-time row / column indices of the Jacobi sweeps cost no scratch and no bank
// conflict (consecutive lanes = consecutive 8-byte words); everything else is indexed at compile time and stays in
// registers.  36 KB of LDS per workgroup: four workgroups per CU.  A hypothesis is a chain of dependent rotations, so
// the launch is bound by LDS latency, not by lanes: K x S = 320 ... 4096 hypotheses spread over 20 ... 256 workgroups
// finish in the time of one.  The eigen-solver is a cyclic Jacobi in a fixed pair order (reproducible run to run); the
// four eigenvectors EPnP reads are those of the four smallest eigenvalues, smallest first (cv::SVD's descending
// order: ut rows 11, 10, 9, 8).  For 4 points that basis is not defined beyond round-off (a 4-dimensional null space);
// see DESIGN.md.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "common.h"
#include "pnp_device.h"
#include "pnp_usun.h"

namespace vieo {

// The two kernels come in two instances: RIG = false, the rectified configuration (G is not read), and RIG = true,
// Frame::usedistort_ (fill_M reads usun, Getuv goes through the correspondence's camera of the rig record in G).

// pass A: job = blockIdx.x * 16 + lane = candidate * n_rows + row; rows of a candidate without a solver (n below
// mRansacMinInliers: iterate never looks at them) are skipped by row_on
template <bool RIG>
__global__ void __launch_bounds__(kPnpLanes)
k_pnp_hypotheses(const PnpCandDev* __restrict__ cands, int n_jobs, int n_rows, const float* __restrict__ Xw,
                 const float* __restrict__ uv, const float* __restrict__ max_err, const int* __restrict__ samples,
                 double* __restrict__ Rt, int* __restrict__ count, unsigned long long* __restrict__ mask, PnpRigArgs G) {
  __shared__ double sA[144 * kPnpLanes], sV[144 * kPnpLanes];
  const int lane = threadIdx.x, job = blockIdx.x * kPnpLanes + lane;
  if (job >= n_jobs) return;
  const PnpCandDev C = cands[job / n_rows];
  if (C.words == 0) return;
  const int row = job % n_rows;
  double R[3][3], t[3];
  pnp_epnp_t<RIG>(C, G, Xw, uv, samples + 4 * (size_t)job, 4, sA, sV, lane, R, t);
  pnp_store_pose(R, t, Rt + 12 * (size_t)job);
  count[job] = pnp_check_inliers_t<RIG>(C, G, Xw, uv, max_err, R, t, mask + C.mask_off + (size_t)row * C.words);
}

// pass B: one record per lane
template <bool RIG>
__global__ void __launch_bounds__(kPnpLanes)
k_pnp_refine(const PnpCandDev* __restrict__ cands, const PnpJob* __restrict__ jobs, int n_jobs,
             const float* __restrict__ Xw, const float* __restrict__ uv, const float* __restrict__ max_err,
             const int* __restrict__ idx, double* __restrict__ Rt, int* __restrict__ count,
             unsigned long long* __restrict__ mask, PnpRigArgs G) {
  __shared__ double sA[144 * kPnpLanes], sV[144 * kPnpLanes];
  const int lane = threadIdx.x, job = blockIdx.x * kPnpLanes + lane;
  if (job >= n_jobs) return;
  const PnpJob J = jobs[job];
  const PnpCandDev C = cands[J.cand];
  double R[3][3], t[3];
  pnp_epnp_t<RIG>(C, G, Xw, uv, idx + J.idx_off, J.cnt, sA, sV, lane, R, t);
  pnp_store_pose(R, t, Rt + 12 * (size_t)job);
  count[job] = pnp_check_inliers_t<RIG>(C, G, Xw, uv, max_err, R, t, mask + J.mask_off);
}

// usun of every correspondence, once per handle: blockIdx.y = candidate, one lane per correspondence
__global__ void __launch_bounds__(64)
k_pnp_usun(const PnpCandDev* __restrict__ cands, const PnpRigDev* __restrict__ rig, const float* __restrict__ uv,
           const unsigned char* __restrict__ cam_of, double* __restrict__ usun) {
  const PnpCandDev C = cands[blockIdx.y];
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= C.n) return;
  const size_t g = (size_t)C.off + i;
  pnp_usun(*rig, cam_of[g], uv[2 * g], uv[2 * g + 1], C.fx, C.fy, C.cx, C.cy, usun + 2 * g);
}


}  // namespace vieo

// ------------------------------------------------------------------------------------------------------------------
// host: the handle vieo_pnp (its tables and the replay of iterate: ransac_table.h), staging and launches
#include <memory>

#include "ransac_table.h"

namespace vieo {

struct PnpScratch {
  DevBuf cands, xw, uv, me, smp, rt, cnt, mask, jobs, idx;
  DevBuf rig, cam, usun;  // the rig instances only
};
static thread_local PnpScratch g_pnp;

// vieo_pnp_rig -> PnpRigDev; false: n_cams outside 1..4 or an unknown camera model
static bool pnp_rig_record(const vieo_pnp_rig& R, PnpRigDev& D) {
  if (R.n_cams < 1 || R.n_cams > 4) return false;
  memset((void*)&D, 0, sizeof(D));
  D.n_cams = R.n_cams;
  for (int c = 0; c < R.n_cams; c++) {
    if (!cam_from_abi(R.cams[c], D.cams[c])) return false;
    memcpy(D.Tcr[c], R.Tcr[c], sizeof(D.Tcr[c])), memcpy(D.Trc[c], R.Trc[c], sizeof(D.Trc[c]));
  }
  return true;
}

// the rig instances' inputs on the device: the record, mapidx2cami_ of n_all correspondences, usun (k_pnp_usun; cd is
// already uploaded, uv too).  max_n: the longest candidate.
static int pnp_rig_stage(const PnpRigDev& rig, const uint8_t* cam_all, size_t n_all, int K, int max_n, PnpRigArgs& A) {
  PnpScratch& G = g_pnp;
  int rc;
  if ((rc = dev_put(G.rig, &rig, sizeof(PnpRigDev))) != VIEO_OK || (rc = dev_put(G.cam, cam_all, n_all)) != VIEO_OK ||
      (rc = G.usun.ensure(n_all * 16)) != VIEO_OK)
    return rc;
  hipLaunchKernelGGL(k_pnp_usun, dim3((unsigned)((max_n + 63) / 64), (unsigned)K), dim3(64), 0, nullptr,
                     G.cands.as<PnpCandDev>(), G.rig.as<PnpRigDev>(), G.uv.as<float>(), G.cam.as<unsigned char>(),
                     G.usun.as<double>());
  VIEO_HIP_CHECK(hipGetLastError());
  A = PnpRigArgs{G.rig.as<PnpRigDev>(), G.cam.as<unsigned char>(), G.usun.as<double>()};
  return VIEO_OK;
}

// pass B over the nj jobs staged in g_pnp (the inputs, jobs, idx), and its tables back: Rt[nj][12], count[nj], mask[words]
static int pnp_refine(bool rig, size_t nj, size_t words, const PnpRigArgs& RA, double* Rt, int32_t* count, uint64_t* mask) {
  PnpScratch& G = g_pnp;
  int rc;
  if ((rc = G.rt.ensure(nj * 96)) != VIEO_OK || (rc = G.cnt.ensure(nj * 4)) != VIEO_OK || (rc = G.mask.ensure(words * 8)) != VIEO_OK)
    return rc;
  hipLaunchKernelGGL(rig ? k_pnp_refine<true> : k_pnp_refine<false>, dim3((unsigned)((nj + kPnpLanes - 1) / kPnpLanes)),
                     dim3(kPnpLanes), 0, nullptr, G.cands.as<PnpCandDev>(), G.jobs.as<PnpJob>(), (int)nj, G.xw.as<float>(),
                     G.uv.as<float>(), G.me.as<float>(), G.idx.as<int>(), G.rt.as<double>(), G.cnt.as<int>(),
                     G.mask.as<unsigned long long>(), RA);
  VIEO_HIP_CHECK(hipGetLastError());
  if ((rc = dev_get(Rt, G.rt, nj * 96)) != VIEO_OK || (rc = dev_get(count, G.cnt, nj * 4)) != VIEO_OK) return rc;
  return dev_get(mask, G.mask, words * 8);
}

// rig == nullptr: the rectified configuration
static int pnp_build(vieo_pnp& H, const vieo_pnp_candidate* cands, int K, const vieo_pnp_params& P,
                     const uint8_t* const* cam_of, const PnpRigDev* rig) {
  const int S = H.n_rows;
  int rc = require_device();
  if (rc != VIEO_OK) return rc;
  // ---- concatenated inputs
  const RansacLayout L = H.layout();
  std::vector<PnpCandDev> cd(K);
  for (int c = 0; c < K; c++)
    cd[c] = PnpCandDev{L.off[c], H.cands[c].n, cands[c].fx, cands[c].fy, cands[c].cx, cands[c].cy, L.words[c], L.mask_off[c]};
  if (L.words_all == 0) return VIEO_OK;  // no candidate has a solver: nothing to compute
  std::vector<float> xw(3 * L.n_all), uv(2 * L.n_all), me(L.n_all);
  for (int c = 0; c < K; c++) {
    const size_t off = cd[c].off, n = cd[c].n;
    if (!n) continue;
    memcpy(&xw[3 * off], cands[c].Xw, n * 12), memcpy(&uv[2 * off], cands[c].uv, n * 8);
    for (size_t i = 0; i < n; i++) me[off + i] = cands[c].sigma2[i] * P.th2;  // mvMaxError, float
  }
  PnpScratch& G = g_pnp;
  const size_t jobsA = (size_t)K * S;
  if ((rc = dev_put(G.cands, cd.data(), K * sizeof(PnpCandDev))) != VIEO_OK || (rc = dev_put(G.xw, xw.data(), xw.size() * 4)) != VIEO_OK ||
      (rc = dev_put(G.uv, uv.data(), uv.size() * 4)) != VIEO_OK || (rc = dev_put(G.me, me.data(), me.size() * 4)) != VIEO_OK ||
      (rc = dev_put(G.smp, H.samples.data(), jobsA * 16)) != VIEO_OK || (rc = dev_zero(G.rt, jobsA * 96)) != VIEO_OK ||
      (rc = dev_zero(G.cnt, jobsA * 4)) != VIEO_OK || (rc = G.mask.ensure(L.words_all * 8)) != VIEO_OK)
    return rc;
  PnpRigArgs RA{nullptr, nullptr, nullptr};
  if (rig) {  // ---- usun
    std::vector<uint8_t> cam_all(L.n_all);
    int max_n = 1;
    for (int c = 0; c < K; c++) {
      if (cd[c].n) memcpy(&cam_all[cd[c].off], cam_of[c], cd[c].n);
      max_n = std::max(max_n, cd[c].n);
    }
    if ((rc = pnp_rig_stage(*rig, cam_all.data(), L.n_all, K, max_n, RA)) != VIEO_OK) return rc;
    std::vector<double> usun(2 * L.n_all);
    if ((rc = dev_get(usun.data(), G.usun, L.n_all * 16)) != VIEO_OK) return rc;
    for (int c = 0; c < K; c++)
      H.cands[c].usun.assign(usun.begin() + 2 * (size_t)cd[c].off, usun.begin() + 2 * ((size_t)cd[c].off + cd[c].n));
  }
  // ---- pass A
  hipLaunchKernelGGL(rig ? k_pnp_hypotheses<true> : k_pnp_hypotheses<false>, dim3((unsigned)((jobsA + kPnpLanes - 1) / kPnpLanes)),
                     dim3(kPnpLanes), 0, nullptr, G.cands.as<PnpCandDev>(), (int)jobsA, S, G.xw.as<float>(), G.uv.as<float>(),
                     G.me.as<float>(), G.smp.as<int>(), G.rt.as<double>(), G.cnt.as<int>(), G.mask.as<unsigned long long>(), RA);
  VIEO_HIP_CHECK(hipGetLastError());
  std::vector<double> rt(jobsA * 12);
  std::vector<int32_t> cnt(jobsA);
  std::vector<uint64_t> mask(L.words_all);
  if ((rc = dev_get(rt.data(), G.rt, jobsA * 96)) != VIEO_OK || (rc = dev_get(cnt.data(), G.cnt, jobsA * 4)) != VIEO_OK ||
      (rc = dev_get(mask.data(), G.mask, L.words_all * 8)) != VIEO_OK)
    return rc;
  for (int c = 0; c < K; c++)
    if (H.cands[c].alive) H.cands[c].slice(c, S, L.mask_off[c], rt.data(), cnt.data(), mask.data());
  // ---- the records: rows that raise the best-so-far set
  std::vector<PnpJob> jobs;
  std::vector<int32_t> idx;
  size_t rec_words;
  pnp_select_records(H, jobs, idx, rec_words);
  const size_t nj = jobs.size();
  if (nj == 0) return VIEO_OK;
  // ---- pass B
  rt.resize(nj * 12), cnt.resize(nj), mask.resize(rec_words);
  if ((rc = dev_put(G.jobs, jobs.data(), nj * sizeof(PnpJob))) != VIEO_OK || (rc = dev_put(G.idx, idx.data(), idx.size() * 4)) != VIEO_OK ||
      (rc = pnp_refine(rig != nullptr, nj, rec_words, RA, rt.data(), cnt.data(), mask.data())) != VIEO_OK)
    return rc;
  pnp_store_records(H, jobs, rt.data(), cnt.data(), mask.data());
  return VIEO_OK;
}

}  // namespace vieo

extern "C" {

// both constructors; rig == nullptr: the rectified configuration
static int pnp_create(vieo_pnp** out, const vieo_pnp_candidate* cands, int n_cands, const uint8_t* const* cam_of,
                      const vieo_pnp_rig* rig, const vieo_pnp_params* params, const int32_t* samples, int n_rows,
                      uint64_t seed) {
  using namespace vieo;
  if (!out) return VIEO_E_INVALID;
  *out = nullptr;
  if (!cands || n_cands <= 0 || !params || n_rows <= 0) {
    set_error("PnPsolver: null argument, no candidate or no sample row");
    return VIEO_E_INVALID;
  }
  if (n_rows > kPnpMaxRows) {
    set_error("PnPsolver: %d sample rows, at most %d", n_rows, kPnpMaxRows);
    return VIEO_E_INVALID;
  }
  if (params->min_set != 4 || !(params->probability > 0 && params->probability < 1) || params->max_iterations < 1 ||
      !(params->epsilon > 0) || params->min_inliers < 0) {
    set_error("PnPsolver: RANSAC parameters out of range (the minimal set is 4 points)");
    return VIEO_E_INVALID;
  }
  for (int c = 0; c < n_cands; c++) {
    const vieo_pnp_candidate& C = cands[c];
    if (C.n < 0 || C.n_frame_keys < 0 || (C.n > 0 && (!C.Xw || !C.uv || !C.sigma2 || !C.key_index))) {
      set_error("PnPsolver: candidate %d is inconsistent", c);
      return VIEO_E_INVALID;
    }
    for (int i = 0; i < C.n; i++)
      if (C.key_index[i] < 0 || C.key_index[i] >= C.n_frame_keys) {
        set_error("PnPsolver: candidate %d, key index %d outside the frame's %d keys", c, C.key_index[i], C.n_frame_keys);
        return VIEO_E_INVALID;
      }
  }
  PnpRigDev rd;
  if (rig) {
    if (!cam_of || !pnp_rig_record(*rig, rd)) {
      set_error("PnPsolver: the rig is inconsistent (1..4 cameras, known models, a camera list per candidate)");
      return VIEO_E_INVALID;
    }
    for (int c = 0; c < n_cands; c++)
      for (int i = 0; i < cands[c].n; i++)
        if (!cam_of[c] || cam_of[c][i] >= rig->n_cams) {
          set_error("PnPsolver: candidate %d, correspondence %d: no camera list or a camera outside the rig's %d", c, i, rig->n_cams);
          return VIEO_E_INVALID;
        }
  }
  std::unique_ptr<vieo_pnp> H(new vieo_pnp);
  H->n_rows = n_rows;
  H->rig = rig != nullptr;
  H->cands.resize(n_cands);
  for (int c = 0; c < n_cands; c++) {
    H->cands[c].set(cands[c].n, cands[c].n_frame_keys, cands[c].key_index);
    pnp_set_ransac_parameters(H->cands[c], *params);
  }
  RansacBadSample bad;
  if (!H->fill_samples(samples, seed, bad)) {
    set_error("PnPsolver: candidate %d, sample row %d: index %d out of range or drawn twice", bad.cand, bad.row, bad.index);
    return VIEO_E_INVALID;
  }
  const int rc = pnp_build(*H, cands, n_cands, *params, cam_of, rig ? &rd : nullptr);
  if (rc == VIEO_OK) *out = H.release();
  return rc;
}

int vieo_pnp_create(vieo_pnp** out, const vieo_pnp_candidate* cands, int n_cands, const vieo_pnp_params* params,
                    const int32_t* samples, int n_rows, uint64_t seed) {
  return pnp_create(out, cands, n_cands, nullptr, nullptr, params, samples, n_rows, seed);
}

int vieo_pnp_create_rig(vieo_pnp** out, const vieo_pnp_candidate* cands, int n_cands, const uint8_t* const* cam_of,
                        const vieo_pnp_rig* rig, const vieo_pnp_params* params, const int32_t* samples, int n_rows,
                        uint64_t seed) {
  if (out) *out = nullptr;
  if (!rig) {
    vieo::set_error("PnPsolver: no rig");
    return VIEO_E_INVALID;
  }
  return pnp_create(out, cands, n_cands, cam_of, rig, params, samples, n_rows, seed);
}

int vieo_pnp_tap_usun(const vieo_pnp* h, int cand, double* usun) {
  if (!h || !h->rig || !h->has(cand) || !usun) return VIEO_E_INVALID;
  const vieo::PnpCand& Q = h->cands[cand];
  if (Q.usun.size() != 2 * (size_t)Q.n) return VIEO_E_INVALID;  // (no candidate had a solver: nothing was computed)
  if (Q.n) memcpy(usun, Q.usun.data(), Q.usun.size() * sizeof(double));
  return VIEO_OK;
}

void vieo_pnp_destroy(vieo_pnp* h) { delete h; }

int vieo_pnp_get_info(const vieo_pnp* h, int cand, vieo_pnp_info* info) {
  if (!h || !info || !h->has(cand)) return VIEO_E_INVALID;
  const vieo::PnpCand& Q = h->cands[cand];
  info->n = Q.n, info->n_frame_keys = Q.n_out, info->min_inliers = Q.min_inliers, info->max_its = Q.max_its;
  info->n_rows = h->n_rows, info->n_records = (int32_t)Q.rec_row.size(), info->mask_words = Q.words;
  info->iterations = Q.iterations, info->best_inliers = Q.best_inliers, info->best_row = Q.best_row;
  return VIEO_OK;
}

int vieo_pnp_iterate(vieo_pnp* h, int cand, int n_iterations, int32_t* found, float* Tcw, uint8_t* inliers,
                     int32_t* n_inliers, int32_t* no_more, int32_t* row_used) {
  if (!h || !h->has(cand) || !found || !Tcw || !n_inliers || !no_more || (h->cands[cand].n_out > 0 && !inliers)) return VIEO_E_INVALID;
  return vieo::pnp_iterate(*h, cand, n_iterations, found, Tcw, inliers, n_inliers, no_more, row_used);
}

int vieo_pnp_tap_rows(const vieo_pnp* h, int cand, int32_t* samples, double* Rt, int32_t* count, uint64_t* mask) {
  return h && h->has(cand) ? h->tap_rows(cand, samples, Rt, count, mask) : VIEO_E_INVALID;
}

int vieo_pnp_tap_records(const vieo_pnp* h, int cand, int32_t* rec_row, double* Rt, int32_t* count, uint64_t* mask) {
  if (!h || !h->has(cand)) return VIEO_E_INVALID;
  const vieo::PnpCand& Q = h->cands[cand];
  const size_t n = Q.rec_row.size();
  if (rec_row && n) memcpy(rec_row, Q.rec_row.data(), n * 4);
  if (Rt && n) memcpy(Rt, Q.rec_Rt.data(), n * 96);
  if (count && n) memcpy(count, Q.rec_count.data(), n * 4);
  if (mask && n) memcpy(mask, Q.rec_mask.data(), n * Q.words * 8);
  return VIEO_OK;
}

static int pnp_tap_refine(const vieo_pnp_candidate* cand, const uint8_t* cam_of, const vieo_pnp_rig* rig,
                          const vieo_pnp_params* params, const uint64_t* masks, int n_masks, double* Rt, int32_t* count,
                          uint64_t* out_masks) {
  using namespace vieo;
  if (!cand || !params || !masks || n_masks <= 0 || !Rt || !count || !out_masks || cand->n < 4 || !cand->Xw || !cand->uv ||
      !cand->sigma2)
    return VIEO_E_INVALID;
  const int n = cand->n, words = (n + 63) / 64;
  PnpRigDev rd;
  if (rig) {
    if (!cam_of || !pnp_rig_record(*rig, rd)) return VIEO_E_INVALID;
    for (int i = 0; i < n; i++)
      if (cam_of[i] >= rig->n_cams) return VIEO_E_INVALID;
  }
  std::vector<PnpJob> jobs;
  std::vector<int32_t> idx;
  for (int m = 0; m < n_masks; m++) {
    const int first = (int)idx.size();
    mask_indices(masks + (size_t)m * words, n, idx);
    if ((int)idx.size() - first < 4) {
      set_error("PnPsolver: mask %d has fewer than 4 correspondences", m);
      return VIEO_E_INVALID;
    }
    jobs.push_back(PnpJob{0, first, (int)idx.size() - first, m * words});
  }
  int rc = require_device();
  if (rc != VIEO_OK) return rc;
  const PnpCandDev cd{0, n, cand->fx, cand->fy, cand->cx, cand->cy, words, 0};
  std::vector<float> me(n);
  for (int i = 0; i < n; i++) me[i] = cand->sigma2[i] * params->th2;
  PnpScratch& G = g_pnp;
  const size_t nj = jobs.size();
  if ((rc = dev_put(G.cands, &cd, sizeof(cd))) != VIEO_OK || (rc = dev_put(G.xw, cand->Xw, (size_t)n * 12)) != VIEO_OK ||
      (rc = dev_put(G.uv, cand->uv, (size_t)n * 8)) != VIEO_OK || (rc = dev_put(G.me, me.data(), (size_t)n * 4)) != VIEO_OK ||
      (rc = dev_put(G.jobs, jobs.data(), nj * sizeof(PnpJob))) != VIEO_OK || (rc = dev_put(G.idx, idx.data(), idx.size() * 4)) != VIEO_OK)
    return rc;
  PnpRigArgs RA{nullptr, nullptr, nullptr};
  if (rig && (rc = pnp_rig_stage(rd, cam_of, (size_t)n, 1, n, RA)) != VIEO_OK) return rc;
  return pnp_refine(rig != nullptr, nj, nj * words, RA, Rt, count, out_masks);
}

int vieo_pnp_tap_refine(const vieo_pnp_candidate* cand, const vieo_pnp_params* params, const uint64_t* masks, int n_masks,
                        double* Rt, int32_t* count, uint64_t* out_masks) {
  return pnp_tap_refine(cand, nullptr, nullptr, params, masks, n_masks, Rt, count, out_masks);
}

int vieo_pnp_tap_refine_rig(const vieo_pnp_candidate* cand, const uint8_t* cam_of, const vieo_pnp_rig* rig,
                            const vieo_pnp_params* params, const uint64_t* masks, int n_masks, double* Rt, int32_t* count,
                            uint64_t* out_masks) {
  if (!rig) return VIEO_E_INVALID;
  return pnp_tap_refine(cand, cam_of, rig, params, masks, n_masks, Rt, count, out_masks);
}

}  // extern "C"
