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
// host: the handle
struct vieo_pnp {
  struct Cand {
    int n = 0, n_frame_keys = 0, words = 0;
    int min_inliers = 0, max_its = 0;
    bool alive = false;  // N >= mRansacMinInliers
    std::vector<int32_t> key_index;
    // pass A tables [n_rows]
    std::vector<double> Rt;
    std::vector<int32_t> count;
    std::vector<uint64_t> mask;
    std::vector<int32_t> rec_of_row;  // the record a row opens, -1 none
    // pass B tables [n_records]
    std::vector<int32_t> rec_row;
    std::vector<double> rec_Rt;
    std::vector<int32_t> rec_count;
    std::vector<uint64_t> rec_mask;
    // PnPsolver's state between iterate calls
    int iterations = 0, best_inliers = 0, best_row = -1, best_rec = -1;
    std::vector<double> usun;  // [n][2], handles of vieo_pnp_create_rig (test tap)
  };
  std::vector<Cand> cands;
  std::vector<int32_t> samples;  // [K][S][4]
  int n_rows = 0;
  bool rig = false;
};

namespace vieo {

// the library's own draw when the caller passes no table: a counter-based generator (splitmix64 of seed, candidate,
// row, draw), k indices without replacement in the reference's swap-with-back manner (PnPsolver.cc:174-186); the Sim3
// solver draws its 3 the same way (declared in common.h)
static inline uint64_t pnp_mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

void pnp_draw(uint64_t seed, int cand, int row, int n, int k, int32_t* out) {
  std::vector<int32_t> avail(n);
  for (int i = 0; i < n; i++) avail[i] = i;
  for (int i = 0; i < k; i++) {
    const uint64_t r = pnp_mix(pnp_mix(seed ^ ((uint64_t)cand << 40)) + ((uint64_t)row << 2) + i);
    const int j = (int)(r % (uint64_t)avail.size());
    out[i] = avail[j];
    avail[j] = avail.back();
    avail.pop_back();
  }
}

// SetRansacParameters (PnPsolver.cc:115-147)
static void pnp_ransac_parameters(const vieo_pnp_params& P, int N, int& min_inliers, int& max_its) {
  float epsilon = P.epsilon;
  int nMinInliers = (int)((float)N * epsilon);
  if (nMinInliers < P.min_inliers) nMinInliers = P.min_inliers;
  if (nMinInliers < P.min_set) nMinInliers = P.min_set;
  min_inliers = nMinInliers;
  if (epsilon < (float)min_inliers / N) epsilon = (float)min_inliers / N;
  int nIterations;
  if (min_inliers == N)
    nIterations = 1;
  else {
    const double its = std::ceil(std::log(1 - P.probability) / std::log(1 - std::pow((double)epsilon, 3.0)));
    nIterations = !(its < 2147483647.0) ? 2147483647 : its < 1.0 ? 1 : (int)its;  // (a NaN or a value below 1 ends as 1 or the cap below)
  }
  max_its = std::max(1, std::min(nIterations, P.max_iterations));
}

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
  if ((rc = G.rig.ensure(sizeof(PnpRigDev))) != VIEO_OK || (rc = G.cam.ensure(n_all)) != VIEO_OK ||
      (rc = G.usun.ensure(n_all * 16)) != VIEO_OK)
    return rc;
  VIEO_HIP_CHECK(hipMemcpy(G.rig.p, &rig, sizeof(PnpRigDev), hipMemcpyHostToDevice));
  VIEO_HIP_CHECK(hipMemcpy(G.cam.p, cam_all, n_all, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_pnp_usun, dim3((unsigned)((max_n + 63) / 64), (unsigned)K), dim3(64), 0, nullptr,
                     G.cands.as<PnpCandDev>(), G.rig.as<PnpRigDev>(), G.uv.as<float>(), G.cam.as<unsigned char>(),
                     G.usun.as<double>());
  VIEO_HIP_CHECK(hipGetLastError());
  A = PnpRigArgs{G.rig.as<PnpRigDev>(), G.cam.as<unsigned char>(), G.usun.as<double>()};
  return VIEO_OK;
}

// pass B over the nj jobs staged in g_pnp
static int pnp_launch_refine(bool rig, size_t nj, const PnpRigArgs& RA) {
  PnpScratch& G = g_pnp;
  const dim3 grid((unsigned)((nj + kPnpLanes - 1) / kPnpLanes));
  if (rig)
    hipLaunchKernelGGL(k_pnp_refine<true>, grid, dim3(kPnpLanes), 0, nullptr, G.cands.as<PnpCandDev>(), G.jobs.as<PnpJob>(),
                       (int)nj, G.xw.as<float>(), G.uv.as<float>(), G.me.as<float>(), G.idx.as<int>(), G.rt.as<double>(),
                       G.cnt.as<int>(), G.mask.as<unsigned long long>(), RA);
  else
    hipLaunchKernelGGL(k_pnp_refine<false>, grid, dim3(kPnpLanes), 0, nullptr, G.cands.as<PnpCandDev>(), G.jobs.as<PnpJob>(),
                       (int)nj, G.xw.as<float>(), G.uv.as<float>(), G.me.as<float>(), G.idx.as<int>(), G.rt.as<double>(),
                       G.cnt.as<int>(), G.mask.as<unsigned long long>(), RA);
  VIEO_HIP_CHECK(hipGetLastError());
  return VIEO_OK;
}

// rig == nullptr: the rectified configuration
static int pnp_build(vieo_pnp& H, const vieo_pnp_candidate* cands, int K, const vieo_pnp_params& P,
                     const uint8_t* const* cam_of, const PnpRigDev* rig) {
  const int S = H.n_rows;
  int rc = require_device();
  if (rc != VIEO_OK) return rc;
  // ---- concatenated inputs
  std::vector<PnpCandDev> cd(K);
  size_t n_all = 0, words_all = 0;
  for (int c = 0; c < K; c++) {
    vieo_pnp::Cand& Q = H.cands[c];
    cd[c] = PnpCandDev{(int)n_all, Q.n, cands[c].fx, cands[c].fy, cands[c].cx, cands[c].cy, Q.alive ? Q.words : 0,
                       (int)words_all};
    n_all += Q.n;
    if (Q.alive) words_all += (size_t)S * Q.words;
  }
  if (words_all == 0) return VIEO_OK;  // no candidate has a solver: nothing to compute
  std::vector<float> xw(3 * n_all), uv(2 * n_all), me(n_all);
  for (int c = 0; c < K; c++) {
    const size_t off = cd[c].off, n = cd[c].n;
    if (!n) continue;
    memcpy(&xw[3 * off], cands[c].Xw, n * 12), memcpy(&uv[2 * off], cands[c].uv, n * 8);
    for (size_t i = 0; i < n; i++) me[off + i] = cands[c].sigma2[i] * P.th2;  // mvMaxError, float
  }
  PnpScratch& G = g_pnp;
  const size_t jobsA = (size_t)K * S;
  if ((rc = G.cands.ensure(K * sizeof(PnpCandDev))) != VIEO_OK || (rc = G.xw.ensure(xw.size() * 4)) != VIEO_OK ||
      (rc = G.uv.ensure(uv.size() * 4)) != VIEO_OK || (rc = G.me.ensure(me.size() * 4)) != VIEO_OK ||
      (rc = G.smp.ensure(jobsA * 16)) != VIEO_OK || (rc = G.rt.ensure(jobsA * 96)) != VIEO_OK ||
      (rc = G.cnt.ensure(jobsA * 4)) != VIEO_OK || (rc = G.mask.ensure(words_all * 8)) != VIEO_OK)
    return rc;
  VIEO_HIP_CHECK(hipMemcpy(G.cands.p, cd.data(), K * sizeof(PnpCandDev), hipMemcpyHostToDevice));
  VIEO_HIP_CHECK(hipMemcpy(G.xw.p, xw.data(), xw.size() * 4, hipMemcpyHostToDevice));
  VIEO_HIP_CHECK(hipMemcpy(G.uv.p, uv.data(), uv.size() * 4, hipMemcpyHostToDevice));
  VIEO_HIP_CHECK(hipMemcpy(G.me.p, me.data(), me.size() * 4, hipMemcpyHostToDevice));
  VIEO_HIP_CHECK(hipMemcpy(G.smp.p, H.samples.data(), jobsA * 16, hipMemcpyHostToDevice));
  VIEO_HIP_CHECK(hipMemset(G.rt.p, 0, jobsA * 96));
  VIEO_HIP_CHECK(hipMemset(G.cnt.p, 0, jobsA * 4));
  PnpRigArgs RA{nullptr, nullptr, nullptr};
  if (rig) {  // ---- usun
    std::vector<uint8_t> cam_all(n_all);
    int max_n = 1;
    for (int c = 0; c < K; c++) {
      if (cd[c].n) memcpy(&cam_all[cd[c].off], cam_of[c], cd[c].n);
      max_n = std::max(max_n, cd[c].n);
    }
    if ((rc = pnp_rig_stage(*rig, cam_all.data(), n_all, K, max_n, RA)) != VIEO_OK) return rc;
    std::vector<double> usun(2 * n_all);
    VIEO_HIP_CHECK(hipMemcpy(usun.data(), G.usun.p, n_all * 16, hipMemcpyDeviceToHost));
    for (int c = 0; c < K; c++)
      H.cands[c].usun.assign(usun.begin() + 2 * (size_t)cd[c].off, usun.begin() + 2 * ((size_t)cd[c].off + cd[c].n));
  }
  // ---- pass A
  const dim3 gridA((unsigned)((jobsA + kPnpLanes - 1) / kPnpLanes));
  if (rig)
    hipLaunchKernelGGL(k_pnp_hypotheses<true>, gridA, dim3(kPnpLanes), 0, nullptr, G.cands.as<PnpCandDev>(), (int)jobsA, S,
                       G.xw.as<float>(), G.uv.as<float>(), G.me.as<float>(), G.smp.as<int>(), G.rt.as<double>(),
                       G.cnt.as<int>(), G.mask.as<unsigned long long>(), RA);
  else
    hipLaunchKernelGGL(k_pnp_hypotheses<false>, gridA, dim3(kPnpLanes), 0, nullptr, G.cands.as<PnpCandDev>(), (int)jobsA, S,
                       G.xw.as<float>(), G.uv.as<float>(), G.me.as<float>(), G.smp.as<int>(), G.rt.as<double>(),
                       G.cnt.as<int>(), G.mask.as<unsigned long long>(), RA);
  VIEO_HIP_CHECK(hipGetLastError());
  std::vector<double> rt(jobsA * 12);
  std::vector<int32_t> cnt(jobsA);
  std::vector<uint64_t> mask(words_all);
  VIEO_HIP_CHECK(hipMemcpy(rt.data(), G.rt.p, jobsA * 96, hipMemcpyDeviceToHost));
  VIEO_HIP_CHECK(hipMemcpy(cnt.data(), G.cnt.p, jobsA * 4, hipMemcpyDeviceToHost));
  VIEO_HIP_CHECK(hipMemcpy(mask.data(), G.mask.p, words_all * 8, hipMemcpyDeviceToHost));
  // ---- the records: rows that raise the best-so-far set (PnPsolver.cc:194-199)
  std::vector<PnpJob> jobs;
  std::vector<int32_t> idx;
  size_t rec_words = 0;
  for (int c = 0; c < K; c++) {
    vieo_pnp::Cand& Q = H.cands[c];
    if (!Q.alive) continue;
    Q.Rt.assign(rt.begin() + (size_t)c * S * 12, rt.begin() + (size_t)(c + 1) * S * 12);
    Q.count.assign(cnt.begin() + (size_t)c * S, cnt.begin() + (size_t)(c + 1) * S);
    Q.mask.assign(mask.begin() + cd[c].mask_off, mask.begin() + cd[c].mask_off + (size_t)S * Q.words);
    Q.rec_of_row.assign(S, -1);
    int best = 0;
    for (int r = 0; r < S; r++) {
      if (Q.count[r] < Q.min_inliers || Q.count[r] <= best) continue;
      best = Q.count[r];
      Q.rec_of_row[r] = (int)Q.rec_row.size();
      Q.rec_row.push_back(r);
      jobs.push_back(PnpJob{c, (int)idx.size(), Q.count[r], (int)rec_words});
      for (int i = 0; i < Q.n; i++)
        if ((Q.mask[(size_t)r * Q.words + i / 64] >> (i % 64)) & 1) idx.push_back(i);
      rec_words += Q.words;
    }
  }
  const size_t nj = jobs.size();
  if (nj == 0) return VIEO_OK;
  // ---- pass B
  if ((rc = G.jobs.ensure(nj * sizeof(PnpJob))) != VIEO_OK || (rc = G.idx.ensure(idx.size() * 4)) != VIEO_OK ||
      (rc = G.rt.ensure(nj * 96)) != VIEO_OK || (rc = G.cnt.ensure(nj * 4)) != VIEO_OK ||
      (rc = G.mask.ensure(rec_words * 8)) != VIEO_OK)
    return rc;
  VIEO_HIP_CHECK(hipMemcpy(G.jobs.p, jobs.data(), nj * sizeof(PnpJob), hipMemcpyHostToDevice));
  VIEO_HIP_CHECK(hipMemcpy(G.idx.p, idx.data(), idx.size() * 4, hipMemcpyHostToDevice));
  if ((rc = pnp_launch_refine(rig != nullptr, nj, RA)) != VIEO_OK) return rc;
  rt.resize(nj * 12), cnt.resize(nj), mask.resize(rec_words);
  VIEO_HIP_CHECK(hipMemcpy(rt.data(), G.rt.p, nj * 96, hipMemcpyDeviceToHost));
  VIEO_HIP_CHECK(hipMemcpy(cnt.data(), G.cnt.p, nj * 4, hipMemcpyDeviceToHost));
  VIEO_HIP_CHECK(hipMemcpy(mask.data(), G.mask.p, rec_words * 8, hipMemcpyDeviceToHost));
  for (size_t j = 0; j < nj; j++) {
    vieo_pnp::Cand& Q = H.cands[jobs[j].cand];
    Q.rec_Rt.insert(Q.rec_Rt.end(), rt.begin() + j * 12, rt.begin() + (j + 1) * 12);
    Q.rec_count.push_back(cnt[j]);
    Q.rec_mask.insert(Q.rec_mask.end(), mask.begin() + jobs[j].mask_off, mask.begin() + jobs[j].mask_off + Q.words);
  }
  return VIEO_OK;
}

// Rcw / tcw .convertTo(CV_32F) into a 4 x 4 identity (PnPsolver.cc:200-206, :264-270)
static void pnp_tcw(const double* Rt, float* Tcw) {
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) Tcw[4 * r + c] = (float)Rt[3 * r + c];
    Tcw[4 * r + 3] = (float)Rt[9 + r];
  }
  Tcw[12] = Tcw[13] = Tcw[14] = 0.f, Tcw[15] = 1.f;
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
  vieo_pnp* H = new vieo_pnp;
  H->n_rows = n_rows;
  H->rig = rig != nullptr;
  H->cands.resize(n_cands);
  H->samples.assign((size_t)n_cands * n_rows * 4, 0);
  for (int c = 0; c < n_cands; c++) {
    vieo_pnp::Cand& Q = H->cands[c];
    Q.n = cands[c].n, Q.n_frame_keys = cands[c].n_frame_keys, Q.words = (Q.n + 63) / 64;
    Q.key_index.assign(cands[c].key_index, cands[c].key_index + Q.n);
    if (Q.n > 0) pnp_ransac_parameters(*params, Q.n, Q.min_inliers, Q.max_its);
    Q.alive = Q.n >= 4 && Q.n >= Q.min_inliers;
    if (Q.n > 0 && Q.n < 4) Q.min_inliers = std::max(Q.min_inliers, 4);  // N < mRansacMinInliers: bNoMore at once
    if (!Q.alive) {
      if (Q.n == 0) Q.min_inliers = std::max(params->min_inliers, 4), Q.max_its = 1;
      continue;
    }
    int32_t* dst = &H->samples[(size_t)c * n_rows * 4];
    for (int r = 0; r < n_rows; r++) {
      if (!samples) {
        pnp_draw(seed, c, r, Q.n, 4, dst + 4 * r);
        continue;
      }
      const int32_t* src = samples + ((size_t)c * n_rows + r) * 4;
      for (int i = 0; i < 4; i++) {
        bool ok = src[i] >= 0 && src[i] < Q.n;
        for (int j = 0; ok && j < i; j++) ok = src[j] != src[i];
        if (!ok) {
          set_error("PnPsolver: candidate %d, sample row %d: index %d out of range or drawn twice", c, r, src[i]);
          delete H;
          return VIEO_E_INVALID;
        }
        dst[4 * r + i] = src[i];
      }
    }
  }
  const int rc = pnp_build(*H, cands, n_cands, *params, cam_of, rig ? &rd : nullptr);
  if (rc != VIEO_OK) {
    delete H;
    return rc;
  }
  *out = H;
  return VIEO_OK;
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
  if (!h || !h->rig || cand < 0 || cand >= (int)h->cands.size() || !usun) return VIEO_E_INVALID;
  const vieo_pnp::Cand& Q = h->cands[cand];
  if (Q.usun.size() != 2 * (size_t)Q.n) return VIEO_E_INVALID;  // (no candidate had a solver: nothing was computed)
  if (Q.n) memcpy(usun, Q.usun.data(), Q.usun.size() * sizeof(double));
  return VIEO_OK;
}

void vieo_pnp_destroy(vieo_pnp* h) { delete h; }

int vieo_pnp_get_info(const vieo_pnp* h, int cand, vieo_pnp_info* info) {
  if (!h || !info || cand < 0 || cand >= (int)h->cands.size()) return VIEO_E_INVALID;
  const vieo_pnp::Cand& Q = h->cands[cand];
  info->n = Q.n, info->n_frame_keys = Q.n_frame_keys, info->min_inliers = Q.min_inliers, info->max_its = Q.max_its;
  info->n_rows = h->n_rows, info->n_records = (int32_t)Q.rec_row.size(), info->mask_words = Q.words;
  info->iterations = Q.iterations, info->best_inliers = Q.best_inliers, info->best_row = Q.best_row;
  return VIEO_OK;
}

int vieo_pnp_iterate(vieo_pnp* h, int cand, int n_iterations, int32_t* found, float* Tcw, uint8_t* inliers,
                     int32_t* n_inliers, int32_t* no_more, int32_t* row_used) {
  using namespace vieo;
  if (!h || cand < 0 || cand >= (int)h->cands.size() || !found || !Tcw || !n_inliers || !no_more) return VIEO_E_INVALID;
  vieo_pnp::Cand& Q = h->cands[cand];
  if (Q.n_frame_keys > 0 && !inliers) return VIEO_E_INVALID;
  *found = 0, *n_inliers = 0, *no_more = 0;
  if (row_used) *row_used = -1;
  if (Q.n_frame_keys > 0) memset(inliers, 0, Q.n_frame_keys);  // vbInliers.clear()
  if (Q.n < Q.min_inliers || !Q.alive) {
    *no_more = 1;
    return VIEO_OK;
  }
  auto give = [&](const double* Rt, const uint64_t* mask, int count, int row) {
    *found = 1, *n_inliers = count;
    if (row_used) *row_used = row;
    pnp_tcw(Rt, Tcw);
    memset(inliers, 0, Q.n_frame_keys);
    for (int i = 0; i < Q.n; i++)
      if ((mask[i / 64] >> (i % 64)) & 1) inliers[Q.key_index[i]] = 1;
  };
  int current = 0;
  while (Q.iterations < Q.max_its || current < n_iterations) {
    if (Q.iterations >= h->n_rows) {
      set_error("PnPsolver: candidate %d needs sample row %d, the table has %d", cand, Q.iterations, h->n_rows);
      return VIEO_E_CAPACITY;
    }
    const int row = Q.iterations;
    current++, Q.iterations++;
    if (Q.count[row] < Q.min_inliers) continue;
    if (Q.count[row] > Q.best_inliers) Q.best_inliers = Q.count[row], Q.best_row = row, Q.best_rec = Q.rec_of_row[row];
    const int rec = Q.best_rec;  // Refine works on the best-so-far set, whichever row opened it
    if (Q.rec_count[rec] > Q.min_inliers) {
      give(&Q.rec_Rt[(size_t)rec * 12], &Q.rec_mask[(size_t)rec * Q.words], Q.rec_count[rec], row);
      return VIEO_OK;
    }
  }
  if (Q.iterations >= Q.max_its) {
    *no_more = 1;
    if (Q.best_inliers >= Q.min_inliers)
      give(&Q.Rt[(size_t)Q.best_row * 12], &Q.mask[(size_t)Q.best_row * Q.words], Q.best_inliers, Q.best_row);
  }
  return VIEO_OK;
}

int vieo_pnp_tap_rows(const vieo_pnp* h, int cand, int32_t* samples, double* Rt, int32_t* count, uint64_t* mask) {
  if (!h || cand < 0 || cand >= (int)h->cands.size()) return VIEO_E_INVALID;
  const vieo_pnp::Cand& Q = h->cands[cand];
  const size_t S = h->n_rows;
  if (samples) memcpy(samples, &h->samples[(size_t)cand * S * 4], S * 16);
  if (!Q.alive) {
    if (Rt) memset(Rt, 0, S * 96);
    if (count) memset(count, 0, S * 4);
    if (mask) memset(mask, 0, S * Q.words * 8);
    return VIEO_OK;
  }
  if (Rt) memcpy(Rt, Q.Rt.data(), S * 96);
  if (count) memcpy(count, Q.count.data(), S * 4);
  if (mask) memcpy(mask, Q.mask.data(), S * Q.words * 8);
  return VIEO_OK;
}

int vieo_pnp_tap_records(const vieo_pnp* h, int cand, int32_t* rec_row, double* Rt, int32_t* count, uint64_t* mask) {
  if (!h || cand < 0 || cand >= (int)h->cands.size()) return VIEO_E_INVALID;
  const vieo_pnp::Cand& Q = h->cands[cand];
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
    for (int i = 0; i < n; i++)
      if ((masks[(size_t)m * words + i / 64] >> (i % 64)) & 1) idx.push_back(i);
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
  if ((rc = G.cands.ensure(sizeof(cd))) != VIEO_OK || (rc = G.xw.ensure((size_t)n * 12)) != VIEO_OK ||
      (rc = G.uv.ensure((size_t)n * 8)) != VIEO_OK || (rc = G.me.ensure((size_t)n * 4)) != VIEO_OK ||
      (rc = G.jobs.ensure(nj * sizeof(PnpJob))) != VIEO_OK || (rc = G.idx.ensure(idx.size() * 4)) != VIEO_OK ||
      (rc = G.rt.ensure(nj * 96)) != VIEO_OK || (rc = G.cnt.ensure(nj * 4)) != VIEO_OK ||
      (rc = G.mask.ensure(nj * words * 8)) != VIEO_OK)
    return rc;
  VIEO_HIP_CHECK(hipMemcpy(G.cands.p, &cd, sizeof(cd), hipMemcpyHostToDevice));
  VIEO_HIP_CHECK(hipMemcpy(G.xw.p, cand->Xw, (size_t)n * 12, hipMemcpyHostToDevice));
  VIEO_HIP_CHECK(hipMemcpy(G.uv.p, cand->uv, (size_t)n * 8, hipMemcpyHostToDevice));
  VIEO_HIP_CHECK(hipMemcpy(G.me.p, me.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  VIEO_HIP_CHECK(hipMemcpy(G.jobs.p, jobs.data(), nj * sizeof(PnpJob), hipMemcpyHostToDevice));
  VIEO_HIP_CHECK(hipMemcpy(G.idx.p, idx.data(), idx.size() * 4, hipMemcpyHostToDevice));
  PnpRigArgs RA{nullptr, nullptr, nullptr};
  if (rig && (rc = pnp_rig_stage(rd, cam_of, (size_t)n, 1, n, RA)) != VIEO_OK) return rc;
  if ((rc = pnp_launch_refine(rig != nullptr, nj, RA)) != VIEO_OK) return rc;
  VIEO_HIP_CHECK(hipMemcpy(Rt, G.rt.p, nj * 96, hipMemcpyDeviceToHost));
  VIEO_HIP_CHECK(hipMemcpy(count, G.cnt.p, nj * 4, hipMemcpyDeviceToHost));
  VIEO_HIP_CHECK(hipMemcpy(out_masks, G.mask.p, nj * words * 8, hipMemcpyDeviceToHost));
  return VIEO_OK;
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
