// tracker.hip -- one stereo-inertial frame's tracking as ONE call behind the C-ABI (vieo_track_frame).
//
// What Tracking::Track does per frame in the steady state (reference: src/Tracking.cc:261-378 TrackWithIMU,
// :385-451 PredictNavStateByIMU, :453-488 TrackLocalMapWithIMU, :2308-2370 SearchLocalPoints; Frame::Frame
// src/Frame.cc:259-320, ComputeStereoMatches :451-611) as a chain of launches on the extractor's stream:
//
//   H2D (one block: header, IMU samples, both images, last frame's points)        [+ local-map block when it changed]
//   stream B:  k_imu_preint (one wavefront; runs beside the extraction)  ----event---+
//   stream A:  extract x 2 -> stereo                                                 v
//              k_track_predict   PredictNavStateByIMU: nav_pred, both optimiser problems, Tcw of the search
//              sbp_project -> search(last frame) -> merge -> build_obs -> PoseOptimization
//              after_pose -> mark_held -> local queries (isInFrustum) -> search(local map) -> merge -> build_obs
//              PoseOptimization(bComputeMarg) -> k_track_finish (per-key outlier flags)
//   D2H (three pieces), ONE host synchronisation.
//
// The order-free bookkeeping between the stages is the vieo_track_* glue of track_glue.hip; nothing here computes
// on the host beyond filling the upload block.  The rare wider-window branch (fewer than 20 matches in the first
// search, Tracking.cc:301-309) re-runs the chain from the projection with 2 x th.
// The chain from the projection to k_track_finish is track_run_chain (track_chain.h), shared with tracker_multi.hip; this
// file owns what differs (the rig's projection, the second stream's hand-over, the local-map queries, the copies back).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "orb_internal.h"
#include "track_chain.h"

namespace vieo {

// upload header: everything small the chain reads, one struct so that it travels with the images in one copy
struct TrkHdr {
  vieo_sbp_camera cam;       // Tcw_cur / Tcw_last are written by k_track_predict / k_track_set_pose
  vieo_vio_frame f1, f2;     // base.nav / imu written by k_track_predict, n_obs / obs_begin by k_track_build_obs
                             // (vision-only trackers use f1.base / f2.base as the vieo_pose_frames)
  vieo_navstate nav_ref, nav_last;
  vieo_imu_noise noise;
  double ti, tj, bg[3], ba[3];
  int32_t first[2];
  int32_t npts[4];           // [0] = n_last, [1] = n_last * n_cams (queries of the first search)
  float consts[32];          // inv_sigma2[16], scale[16]
};

// The next frame's pre-integration, run ahead (vieo_track_input.next_imu): what goes up for it.  In HBM the block is
// [SpecImu | samples | bias (6 doubles, written by k_track_predict) | vieo_imu_preint | Sigma_prv (81) | status].
struct SpecImu {
  vieo_imu_noise noise;
  double ti, tj;
  int32_t first[2];
  double xbias[6];  // next_ref_bias: the reference's bias when it is not this frame's predicted one
};

// download header
struct TrkOut {
  int32_t cnt[8];            // extractor counts per image: {n, mono}
  int32_t nm[4];             // [0] matches of the first search, [1] of the second
  int32_t nq[4];
  int32_t preint_status[4];
  vieo_vio_result r1, r2;
  vieo_navstate nav_pred;
  vieo_imu_preint imu;
  double sigma_prv[81];
  int32_t nobs2[4];          // observations of the second optimisation
  int32_t fe_hdr[8];         // rig: header of the stereo stage (groups, matches, threshold, status, ...)
  int32_t cam_first[8];      // rig: first key of every camera in mvKeys, [n_cams] = N
  int32_t fcnt[2];           // rig: {N, 0}
};

// PredictNavStateByIMU (Tracking.cc:385-451) from the pre-integration in HBM; fills the two optimiser problems and
// the projection search's camera (track_predict_frame, shared with the multi-sequence tracker).
__global__ void __launch_bounds__(64)
k_track_predict(TrkHdr* __restrict__ H, TrkOut* __restrict__ O, const vieo_imu_preint* __restrict__ pre,
                const double* __restrict__ sigma_prv, const int32_t* __restrict__ status, double* __restrict__ next_bias,
                TrkTables tables) {
  if (blockIdx.x > 0) return track_fill_tables(tables, H->npts[0]);
  __shared__ vieo_navstate s_nav;
  track_predict_frame(&H->nav_ref, &H->nav_last, &H->f1, &H->f2, &H->cam, &O->nav_pred, &O->imu, O->sigma_prv,
                      O->preint_status, pre, sigma_prv, status, next_bias, s_nav);
}

// The vision-only tracker's prediction comes from the host (mVelocity * mLastFrame.Tcw, Tracking.cc:1852): the two
// optimiser problems start from it, the projection search gets Tcw of it and of the last frame.
__global__ void __launch_bounds__(64)
k_track_set_pose(TrkHdr* __restrict__ H, TrkOut* __restrict__ O, TrkTables tables) {
  if (blockIdx.x > 0) return track_fill_tables(tables, H->npts[0]);
  track_set_pose_frame(&H->nav_ref, &H->nav_last, H->f1.base.Rcb, H->f1.base.tcb, &H->cam, &H->f1.base.nav, &H->f2.base.nav,
                       &O->nav_pred, O->preint_status);
}

// A prefetched frame becomes the current one: the slot the third stream extracted into -> the arrays the chain reads
// (both images' keys and descriptors, their counts, uright / depth of the stereo stage).  One launch instead of five copies.
__global__ void __launch_bounds__(256)
k_track_adopt(const uint4* __restrict__ s_kp, uint4* __restrict__ d_kp, int n_kp16, const uint4* __restrict__ s_desc,
              uint4* __restrict__ d_desc, int n_desc16, const uint4* __restrict__ s_ur, uint4* __restrict__ d_ur,
              const uint4* __restrict__ s_dp, uint4* __restrict__ d_dp, int n_f16, const int32_t* __restrict__ s_cnt,
              int32_t* __restrict__ d_cnt, int n_cnt) {
  const int stride = gridDim.x * 256;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n_kp16; i += stride) d_kp[i] = s_kp[i];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n_desc16; i += stride) d_desc[i] = s_desc[i];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n_f16; i += stride) d_ur[i] = s_ur[i], d_dp[i] = s_dp[i];
  if (blockIdx.x == 0 && threadIdx.x < n_cnt) d_cnt[threadIdx.x] = s_cnt[threadIdx.x];
}

}  // namespace vieo

using namespace vieo;

struct vieo_tracker {
  vieo_tracker_params P;
  vieo_tracker_rig R;
  bool rig = false, vision = false;
  int n_img = 2;     // images per frame
  int nc = 1;        // cameras the searches loop over (1: the rectified pair's left camera)
  int kc = 0;        // key capacity of a frame: cap, or n_cams * cap of a rig (mvKeys)
  vieo_orb* ext = nullptr;
  vieo_fisheye* fe = nullptr;
  hipStream_t st = nullptr, st_imu = nullptr, st_pref = nullptr;
  hipEvent_t ev_up = nullptr, ev_imu = nullptr, ev_t0 = nullptr, ev_t1 = nullptr, ev_ext = nullptr, ev_fe = nullptr, ev_kd = nullptr;
  hipEvent_t ev_head = nullptr, ev_pref = nullptr;  // this frame's stereo stage is done / the next frame is extracted
  hipEvent_t ev_spec = nullptr;                     // the pre-integration run ahead (second stream) is done
  hipEvent_t ev_h2d = nullptr;                      // the prefetched images have left the pinned planes
  bool h2d_pending = false;
  hipEvent_t ev_tab = nullptr;                      // a changed local map (second stream) is in place
  // frame pipelining (vieo_track_input.next_left / next_right): the next frame's images and what its extraction and
  // stereo stage produce, on the third stream
  uint8_t *h_next = nullptr, *d_next = nullptr, *d_slot = nullptr;
  size_t s_kp = 0, s_desc = 0, s_ur = 0, s_dp = 0, s_cnt = 0;
  bool pref_valid = false;
  int pref_frames = 0;
  // ... and its pre-integration (next_imu): pinned / device blocks, what was integrated (the next call compares), counts
  uint8_t *h_spec = nullptr, *d_spec = nullptr;
  size_t sp_samples = 0, sp_bias = 0, sp_pre = 0, sp_prv = 0, sp_pst = 0, sp_up = 0;
  std::vector<vieo_imu_sample> spec_samples;
  double spec_ti = 0, spec_tj = 0, spec_bias[6] = {0, 0, 0, 0, 0, 0};
  int spec_n = 0;
  bool spec_valid = false;
  int spec_used = 0;
  int cap = 0, ccap = 0, pcap = 0, gcap = 0, imu_cap = 512;
  int local_version = -1, n_local_dev = 0;
  int replica_repeats = 0;    // frames whose optimisations were repeated on one workgroup (a replica did not arrive)
  float side_ratio = 0.f;     // create_side_stream: elapsed(both spin kernels) / elapsed(one): 1 side by side, 2 in series
  int side_probes = 1, side_checks = 0;
  // the frames' GPU times: a ring for the running median, and how many frames in a row sat 30 % above it -- the sign that
  // the two streams have come to share a hardware queue (streams the process created since: the mapping is the runtime's)
  float gpu_ring[32] = {};
  int gpu_n = 0, slow_run = 0, frames_since_check = 0;
  float scale[16], inv_sigma2[16];
  TrackConstants K;  // the constant parts of a frame's records (copied into the pinned TrkHdr), the frustum frame, the bounds
  // pinned blocks and their device twins (same layout)
  uint8_t *h_up = nullptr, *d_up = nullptr;      // per-frame upload
  uint8_t *h_loc = nullptr, *d_loc = nullptr;    // local-map candidates (uploaded when they change)
  uint8_t *h_out = nullptr, *d_out = nullptr;    // download
  uint8_t* d_work = nullptr;                     // device-only scratch
  uint8_t* d_const = nullptr;                    // rig: vieo_sbp_rig | vieo_camera[4]
  // offsets in the upload block
  size_t up_bytes, slot_bytes, loc_bytes, work_bytes, spec_bytes, const_bytes, img_bytes;
  size_t o_hdr, o_imu, o_img, o_pts, o_xyz, o_dep, o_alias, up_fixed, up_small;
  // offsets in the local block
  size_t l_cpt, l_cdesc, l_xyz;
  // offsets in the download block
  size_t q_hdr, q_ur, q_dp, q_mpref, q_outl, q_kg, q_gidx, q_good, q_p3d, q_small_end, q_kp, q_desc, q_cdep, out_bytes;
  // offsets in the work block
  size_t w_kp, w_desc, w_kcat, w_dcat, w_q1, w_q1c, w_qsrc, w_q2, w_assign, w_taken, w_held, w_obs, w_obskey, w_outl, w_xyz,
      w_dep, w_pre, w_prv, w_pst;
};

// The second stream of a tracker (pre-integration, a rig frame's stereo bookkeeping, the copies back) must be served by
// another hardware queue than the first: on one queue their kernels run one after the other (observed with two streams
// of equal priority: the "parallel" pre-integration of every frame sat in front of its extraction, 100 us; in a process
// that holds many streams the assignment is anybody's guess: a 2-camera frame 1.06 -> 1.55 ms with eight idle torch
// streams around).  HIP does not say which queue a stream gets, so candidates are TRIED: a ~40 us spin kernel on each of
// the two streams, started together -- a candidate whose kernel ends when the first one's does runs beside it.  High
// priority first (its own pool of queues where the runtime has one), a handful of attempts, the best one is kept.
__global__ void k_track_spin(long long cycles) {
  const long long t0 = __builtin_amdgcn_s_memtime();
  while (__builtin_amdgcn_s_memtime() - t0 < cycles) __builtin_amdgcn_s_sleep(8);
}
// elapsed(both spin kernels, started together on the two streams) / elapsed(one): ~1 side by side, ~2 one after the other
static bool side_stream_ratio(hipStream_t main_stream, hipStream_t c, hipEvent_t e0, hipEvent_t e1, hipEvent_t e2, float* ratio) {
  const long long spin = 100000;  // ~40 us
  float both = 0, one = 0;
  bool ok = true;
  for (int rep = 0; rep < 2 && ok; rep++) {  // (the first round also creates the candidate's queue)
    ok = hipEventRecord(e0, main_stream) == hipSuccess && hipStreamWaitEvent(c, e0, 0) == hipSuccess;
    hipLaunchKernelGGL(k_track_spin, dim3(1), dim3(64), 0, main_stream, spin);
    hipLaunchKernelGGL(k_track_spin, dim3(1), dim3(64), 0, c, spin);
    ok = ok && hipEventRecord(e1, main_stream) == hipSuccess && hipEventRecord(e2, c) == hipSuccess &&
         hipStreamSynchronize(main_stream) == hipSuccess && hipStreamSynchronize(c) == hipSuccess &&
         hipEventElapsedTime(&one, e0, e1) == hipSuccess && hipEventElapsedTime(&both, e0, e2) == hipSuccess;
  }
  if (ok) *ratio = both / (one > 0 ? one : 1.f);
  return ok;
}
static const float kSideRatioOk = 1.35f;
// *ratio: what the kept stream measured (reported by vieo_tracker_get_stats; > kSideRatioOk = no candidate ran beside
// the main stream, the best of them is kept and the frame's second stream is then in series with the first)
hipError_t vieo::create_side_stream(hipStream_t* out, hipStream_t main_stream, float* ratio_out) {
  int lo = 0, hi = 0;
  const bool prio = hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && lo != hi;
  hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
  *ratio_out = 0.f;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess || hipEventCreate(&e2) != hipSuccess) {
    for (hipEvent_t e : {e0, e1, e2})
      if (e) (void)hipEventDestroy(e);
    return prio ? hipStreamCreateWithPriority(out, hipStreamNonBlocking, hi) : hipStreamCreateWithFlags(out, hipStreamNonBlocking);
  }
  hipStream_t best = nullptr, held[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  float best_ratio = 1e9f;
  for (int k = 0; k < 6; k++) {
    hipStream_t c = nullptr;
    // (normal-priority candidates first: the main stream is a high-priority one unless VIEO_TRACKER_PRIORITY=0)
    const hipError_t err = (prio && k % 2 == 1) ? hipStreamCreateWithPriority(&c, hipStreamNonBlocking, hi)
                                                : hipStreamCreateWithFlags(&c, hipStreamNonBlocking);
    if (err != hipSuccess) break;
    held[k] = c;  // (kept until the end: a destroyed candidate's queue would be handed to the next one)
    float ratio = 0;
    if (!side_stream_ratio(main_stream, c, e0, e1, e2, &ratio)) continue;
    if (ratio < best_ratio) best_ratio = ratio, best = c;
    if (ratio < kSideRatioOk) break;
  }
  for (hipStream_t c : held)
    if (c && c != best) (void)hipStreamDestroy(c);
  for (hipEvent_t e : {e0, e1, e2}) (void)hipEventDestroy(e);
  if (!best) return hipErrorUnknown;
  *out = best, *ratio_out = best_ratio;
  return hipSuccess;
}

// The third stream (the next frame's extraction).  VIEO_PREFETCH_PRIORITY = -1 (lowest: the bundle adjustment's pool of
// hardware queues), 0 (normal, the default), 1 (highest): A/B runs.
static hipError_t create_prefetch_stream(hipStream_t* out) {
  const char* e = getenv("VIEO_PREFETCH_PRIORITY");
  const int want = e ? atoi(e) : 0;
  int lo = 0, hi = 0;
  if (want != 0 && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && lo != hi)
    return hipStreamCreateWithPriority(out, hipStreamNonBlocking, want < 0 ? lo : hi);
  return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}

// the running median of the frames' GPU times (0: fewer than min_n frames)
static float track_gpu_median(const vieo_tracker* t, int min_n) {
  const int n = std::min(t->gpu_n, 32);
  if (n < min_n) return 0.f;
  float v[32];
  memcpy(v, t->gpu_ring, sizeof(float) * n);
  std::nth_element(v, v + n / 2, v + n);
  return v[n / 2];
}

// ---- vieo_tracker_create_rig's steps

// the extractor (its stream is the tracker's main stream), a rig's stereo stage, and the capacities they give
static int tracker_open_front_end(vieo_tracker* t, const vieo_tracker_params& P, const vieo_tracker_rig& R) {
  int rc = vieo::orb_create_with_priority(&t->ext, P.n_features, P.scale_factor, P.n_levels, P.ini_th_fast, P.min_th_fast,
                                          track_main_priority());
  if (rc != VIEO_OK) return rc;
  t->st = (hipStream_t)vieo_orb_stream(t->ext);
  t->cap = vieo_orb_max_keypoints(t->ext), t->kc = t->nc * t->cap;
  t->ccap = std::max(P.max_local_points, 64), t->pcap = t->kc + t->ccap;
  vieo_orb_scale_factors(t->ext, t->scale), vieo_orb_inv_level_sigma2(t->ext, t->inv_sigma2);
  if (!t->rig) return VIEO_OK;
  float sig2[16];
  vieo_orb_level_sigma2(t->ext, sig2);
  vieo_fisheye_params fp = {};
  fp.n_cams = R.n_cams, fp.n_levels = P.n_levels, fp.bf = P.bf, fp.th_far_pts = R.th_far_pts;
  fp.cams = R.cams, fp.Trc = &R.Trc[0][0], fp.Tcr = &R.Tcr[0][0], fp.level_sigma2 = sig2;
  if ((rc = vieo_fisheye_create(&t->fe, &fp, t->cap, 1)) != VIEO_OK) return rc;
  t->gcap = vieo_fisheye_group_capacity(t->fe);
  return VIEO_OK;
}

// the offsets of the blocks' arrays and the blocks' sizes
static void tracker_layout(vieo_tracker* t) {
  Layout U, S, L, Q, W, Sp;  // upload, prefetch slot, local map, download, work, run-ahead pre-integration
  const int cap = t->cap, ccap = t->ccap, kc = t->kc, nc = t->nc, rig = t->rig;
  t->img_bytes = (size_t)t->n_img * t->P.width * t->P.height;
  // upload block: [header | IMU samples | last points | their xyz | their depth | alias | images]: the images last, so
  // that a call whose frame was prefetched uploads the head only
  t->o_hdr = U.take(sizeof(TrkHdr)), t->o_imu = U.take((size_t)t->imu_cap * sizeof(vieo_imu_sample));
  t->o_pts = U.take((size_t)kc * sizeof(vieo_last_frame_point));
  t->o_xyz = U.take((size_t)kc * 12), t->o_dep = U.take((size_t)kc * 4), t->o_alias = U.take((size_t)ccap * 4);
  t->up_fixed = t->o_alias, t->up_small = U.o, t->o_img = U.take(t->img_bytes), t->up_bytes = U.o;
  // the prefetch slot: both images' keys / descriptors, counts, uright / depth of the left image
  t->s_kp = S.take((size_t)t->n_img * cap * sizeof(vieo_keypoint)), t->s_desc = S.take((size_t)t->n_img * cap * 32);
  t->s_ur = S.take((size_t)cap * 4 + 16), t->s_dp = S.take((size_t)cap * 4 + 16), t->s_cnt = S.take(64), t->slot_bytes = S.o;
  t->l_cpt = L.take((size_t)ccap * sizeof(vieo_frustum_point)), t->l_cdesc = L.take((size_t)ccap * 32),
      t->l_xyz = L.take((size_t)ccap * 12), t->loc_bytes = L.o;
  t->q_hdr = Q.take(sizeof(TrkOut)), t->q_ur = Q.take((size_t)kc * 4), t->q_dp = Q.take((size_t)kc * 4),
      t->q_mpref = Q.take((size_t)kc * 4), t->q_outl = Q.take(kc);
  t->q_kg = t->q_gidx = t->q_good = t->q_p3d = Q.o;
  if (rig) {
    t->q_kg = Q.take((size_t)kc * 4), t->q_gidx = Q.take((size_t)t->gcap * nc * 4), t->q_good = Q.take(t->gcap),
        t->q_p3d = Q.take((size_t)t->gcap * 24);
  }
  t->q_small_end = Q.o;
  t->q_kp = Q.take((size_t)kc * sizeof(vieo_keypoint)), t->q_desc = Q.take((size_t)kc * 32), t->q_cdep = Q.take((size_t)ccap * 4);
  t->out_bytes = Q.o;
  t->w_kp = W.take((size_t)t->n_img * cap * sizeof(vieo_keypoint)), t->w_desc = W.take((size_t)t->n_img * cap * 32);
  t->w_kcat = t->w_kp, t->w_dcat = t->w_desc;
  if (rig) t->w_kcat = W.take((size_t)kc * sizeof(vieo_keypoint)), t->w_dcat = W.take((size_t)kc * 32);
  t->w_q1 = W.take((size_t)kc * nc * sizeof(vieo_proj_query)), t->w_q2 = W.take((size_t)ccap * nc * sizeof(vieo_proj_query));
  t->w_q1c = t->w_q1, t->w_qsrc = 0;
  if (rig) t->w_q1c = W.take((size_t)kc * nc * sizeof(vieo_proj_query)), t->w_qsrc = W.take((size_t)kc * nc * 4);
  t->w_assign = W.take((size_t)kc * 4), t->w_taken = W.take(kc), t->w_held = W.take(t->pcap);
  t->w_obs = W.take((size_t)kc * sizeof(vieo_pose_obs)), t->w_obskey = W.take((size_t)kc * 4), t->w_outl = W.take(kc);
  t->w_xyz = W.take((size_t)t->pcap * 12), t->w_dep = W.take((size_t)t->pcap * 4);
  t->w_pre = W.take(sizeof(vieo_imu_preint)), t->w_prv = W.take(81 * 8), t->w_pst = W.take(16), t->work_bytes = W.o;
  (void)Sp.take(sizeof(SpecImu));
  t->sp_samples = Sp.take((size_t)t->imu_cap * sizeof(vieo_imu_sample)), t->sp_up = Sp.o;
  t->sp_bias = Sp.take(6 * 8), t->sp_pre = Sp.take(sizeof(vieo_imu_preint)), t->sp_prv = Sp.take(81 * 8), t->sp_pst = Sp.take(16),
      t->spec_bytes = Sp.o;
  t->const_bytes = al256(sizeof(vieo_sbp_rig)) + al256(sizeof(vieo_camera) * 4);
}

// the pinned and device blocks, the second and third stream, the events; the blocks cleared
static bool tracker_allocate(vieo_tracker* t) {
  const auto pinned = [](uint8_t** p, size_t n) { return hipHostMalloc((void**)p, n, hipHostMallocDefault) == hipSuccess; };
  const auto device = [](uint8_t** p, size_t n) { return hipMalloc((void**)p, n) == hipSuccess; };
  bool ok = pinned(&t->h_up, t->up_bytes) && pinned(&t->h_loc, t->loc_bytes) && pinned(&t->h_out, t->out_bytes) &&
      device(&t->d_up, t->up_bytes) &&
            device(&t->d_loc, t->loc_bytes) && device(&t->d_out, t->out_bytes) && device(&t->d_work, t->work_bytes) &&
            device(&t->d_const, t->const_bytes) &&
            pinned(&t->h_spec, t->sp_up) && device(&t->d_spec, t->spec_bytes) && hipMemset(t->d_spec, 0, t->spec_bytes) == hipSuccess &&
            pinned(&t->h_next, t->img_bytes) && device(&t->d_next, t->img_bytes) && device(&t->d_slot, t->slot_bytes) &&
            create_prefetch_stream(&t->st_pref) == hipSuccess;
  for (hipEvent_t* e : {&t->ev_pref, &t->ev_h2d, &t->ev_spec, &t->ev_head, &t->ev_tab})
    ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
  ok = ok && create_side_stream(&t->st_imu, t->st, &t->side_ratio) == hipSuccess;
  for (hipEvent_t* e : {&t->ev_up, &t->ev_imu, &t->ev_ext, &t->ev_fe, &t->ev_kd})
    ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipEventCreate(&t->ev_t0) == hipSuccess && hipEventCreate(&t->ev_t1) == hipSuccess;
  if (!ok) return false;
  memset(t->h_up, 0, t->up_bytes), memset(t->h_loc, 0, t->loc_bytes), memset(t->h_out, 0, t->out_bytes);
  (void)hipMemsetAsync(t->d_work, 0, t->work_bytes, t->st), (void)hipMemsetAsync(t->d_out, 0, t->out_bytes, t->st);
  return true;
}

// the constant parts of the header; rigs: the searches' rig and the cameras go up, once
static int tracker_constants(vieo_tracker* t) {
  const vieo_tracker_rig* R = t->rig ? &t->R : nullptr;
  vieo_camera* d_cams = (vieo_camera*)(t->d_const + al256(sizeof(vieo_sbp_rig)));
  TrackConstants& K = t->K;
  track_build_constants(K, t->P, t->scale, t->inv_sigma2, R, d_cams);
  TrkHdr& H = *(TrkHdr*)(t->h_up + t->o_hdr);
  memcpy(&H.cam, &K.cam0, sizeof(H.cam)), memcpy(&H.f1, &K.f1_0, sizeof(H.f1)), memcpy(&H.f2, &K.f2_0, sizeof(H.f2));
  memcpy(H.consts, K.consts, sizeof(H.consts)), H.noise = t->P.noise;
  if (!R) return VIEO_OK;
  // (Tcr / trc cast to double as mpCameras[c]->GetTcr().cast<double>())
  vieo_sbp_rig sr = {};
  sr.n_cams = R->n_cams, sr.use_distort = 1;
  for (int c = 0; c < R->n_cams; c++) {
    sr.cams[c] = R->cams[c];
    memcpy(sr.Tcr[c], R->Tcr[c], 96);
    for (int r = 0; r < 3; r++) sr.trc[c][r] = R->Trc[c][r * 4 + 3];
    memcpy(sr.bounds[c], K.bounds[c], 16);
  }
  if (hipMemcpy(t->d_const, &sr, sizeof(sr), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_cams, R->cams, sizeof(vieo_camera) * R->n_cams, hipMemcpyHostToDevice) != hipSuccess) {
    set_error("vieo_tracker_create: constant upload failed");
    return VIEO_E_HIP;
  }
  return VIEO_OK;
}

extern "C" {

void vieo_tracker_destroy(vieo_tracker* t) {
  if (!t) return;
  if (t->st) (void)hipStreamSynchronize(t->st);
  if (t->st_imu) (void)hipStreamSynchronize(t->st_imu), (void)hipStreamDestroy(t->st_imu);
  if (t->st_pref) (void)hipStreamSynchronize(t->st_pref), (void)hipStreamDestroy(t->st_pref);
  for (hipEvent_t e : {t->ev_up, t->ev_imu, t->ev_t0, t->ev_t1, t->ev_ext, t->ev_fe, t->ev_kd, t->ev_head, t->ev_pref, t->ev_tab,
                       t->ev_h2d, t->ev_spec})
    if (e) (void)hipEventDestroy(e);
  for (uint8_t* p : {t->h_up, t->h_loc, t->h_out, t->h_next, t->h_spec})
    if (p) (void)hipHostFree(p);
  for (uint8_t* p : {t->d_up, t->d_loc, t->d_out, t->d_work, t->d_const, t->d_next, t->d_slot, t->d_spec})
    if (p) (void)hipFree(p);
  if (t->fe) vieo_fisheye_destroy(t->fe);
  if (t->ext) vieo_orb_destroy(t->ext);
  delete t;
}

int vieo_tracker_create_rig(vieo_tracker** out, const vieo_tracker_params* P, const vieo_tracker_rig* R) {
  if (!out || !P || P->width <= 0 || P->height <= 0 || P->n_levels < 1 || P->n_levels > 16 || P->max_local_points < 0)
    return VIEO_E_INVALID;
  if (R && (R->n_cams < 2 || R->n_cams > 4 || P->vision_only)) {
    set_error("vieo_tracker_create_rig: %d cameras (2..4), visual-inertial", R->n_cams);
    return VIEO_E_INVALID;
  }
  int rc = require_device();
  if (rc != VIEO_OK) return rc;
  vieo_tracker* t = new vieo_tracker();
  t->P = *P, t->rig = R != nullptr, t->vision = P->vision_only != 0, t->n_img = R ? R->n_cams : 2, t->nc = R ? R->n_cams : 1;
  if (R) t->R = *R;
  if ((rc = tracker_open_front_end(t, t->P, t->R)) == VIEO_OK) {
    tracker_layout(t);
    if (tracker_allocate(t))
      rc = tracker_constants(t);
    else
      set_error("vieo_tracker_create: allocation failed (%s)", hipGetErrorString(hipGetLastError())), rc = VIEO_E_HIP;
  }
  if (rc != VIEO_OK) {
    vieo_tracker_destroy(t);
    return rc;
  }
  *out = t;
  return VIEO_OK;
}

int vieo_tracker_create(vieo_tracker** out, const vieo_tracker_params* P) { return vieo_tracker_create_rig(out, P, nullptr); }

int vieo_tracker_image_buffers(vieo_tracker* t, uint8_t** left, uint8_t** right) {
  if (!t || !left || !right) return VIEO_E_INVALID;
  *left = t->h_up + t->o_img;
  *right = *left + (size_t)t->P.width * t->P.height;
  return VIEO_OK;
}

int vieo_tracker_image_buffer(vieo_tracker* t, int image_index, uint8_t** plane) {
  if (!t || !plane || image_index < 0 || image_index >= t->n_img) return VIEO_E_INVALID;
  *plane = t->h_up + t->o_img + (size_t)image_index * t->P.width * t->P.height;
  return VIEO_OK;
}

int vieo_tracker_scale_factors(const vieo_tracker* t, float* h_out) {
  if (!t || !h_out) return VIEO_E_INVALID;
  for (int l = 0; l < t->P.n_levels; l++) h_out[l] = t->scale[l];
  return VIEO_OK;
}

// The second stream again: measured first, replaced only when it no longer runs beside the main one.  Both streams are
// idle here (every vieo_track_frame returns synchronised).
int vieo_tracker_reprobe(vieo_tracker* t) {
  if (!t) return VIEO_E_INVALID;
  int rc = require_device();
  if (rc != VIEO_OK) return rc;
  VIEO_HIP_CHECK(hipStreamSynchronize(t->st));
  VIEO_HIP_CHECK(hipStreamSynchronize(t->st_imu));
  hipEvent_t e[3] = {nullptr, nullptr, nullptr};
  for (auto& ev : e) VIEO_HIP_CHECK(hipEventCreate(&ev));
  float ratio = 0;
  const bool ok = side_stream_ratio(t->st, t->st_imu, e[0], e[1], e[2], &ratio);
  for (auto& ev : e) (void)hipEventDestroy(ev);
  t->side_checks++;
  if (ok) t->side_ratio = ratio;
  if (ok && ratio < kSideRatioOk) return VIEO_OK;
  hipStream_t fresh = nullptr;
  float fr = 0;
  if (create_side_stream(&fresh, t->st, &fr) != hipSuccess) return VIEO_OK;  // (keep what there is)
  if (ok && fr >= ratio) {  // nothing better to be had
    (void)hipStreamDestroy(fresh);
    return VIEO_OK;
  }
  (void)hipStreamDestroy(t->st_imu);
  t->st_imu = fresh, t->side_ratio = fr, t->side_probes++;
  return VIEO_OK;
}

int vieo_tracker_get_stats(const vieo_tracker* t, vieo_tracker_stats* out) {
  if (!t || !out) return VIEO_E_INVALID;
  memset(out, 0, sizeof(*out));
  out->side_stream_ratio = t->side_ratio, out->side_stream_selections = t->side_probes, out->side_stream_checks = t->side_checks;
  out->replica_repeats = t->replica_repeats;
  out->frames_prefetched = t->pref_frames, out->preints_ahead_used = t->spec_used;
  out->ms_gpu_median = track_gpu_median(t, 1);
  out->slow_frames_in_a_row = t->slow_run;
  return VIEO_OK;
}

int vieo_tracker_key_capacity(const vieo_tracker* t) { return t ? t->kc : 0; }
int vieo_tracker_group_capacity(const vieo_tracker* t) { return t ? t->gcap : 0; }

int vieo_tracker_get_level(vieo_tracker* t, int image_index, int level, int with_border, uint8_t* h_dst, int dst_stride) {
  if (!t) return VIEO_E_INVALID;
  return vieo_orb_get_level(t->ext, image_index, level, with_border, h_dst, dst_stride);
}

}  // extern "C"

// ---- vieo_track_frame: a call record and the stages that work on it
struct TrackCall {
  vieo_tracker* t;
  const vieo_track_input* in;
  vieo_track_output* out;
  const uint8_t *imgs[4] = {}, *nx[4] = {};  // this frame's images; the next frame's, if the caller has them
  int nl = 0, nc = 0, n_next = 0;            // last-frame points, local-map candidates, next images given (0 or all)
  bool pref = false, new_local = false;      // the frame was extracted by the previous call; the local map changed
  bool spec = false, spec_ref = false;       // next_imu is integrated ahead: from this frame / from the reference the caller names
  int widened = 0;
  TrkHdr *H, *dH;                            // upload header: pinned, device
  TrkOut* dO;                                // download header: device; O: pinned
  const TrkOut* O;
  vieo_keypoint* d_kp;                       // what the extraction writes: n_img x cap keys, d_desc: descriptors
  uint8_t* d_desc;
  hipStream_t s_head;                        // where the prediction and the projection run
  TrackChain chain;
  std::chrono::steady_clock::time_point t_enter;
};

// the tracker's arrays as the chain reads them (one frame)
static TrackChain track_chain_of(vieo_tracker* t, TrkHdr* dH, TrkOut* dO) {
  const int kc = t->kc, nc = t->nc;
  uint8_t *W = t->d_work, *Q = t->d_out;
  TrackChain c;
  c.n = 1, c.kc = kc, c.pcap = t->pcap, c.n_cams = nc, c.rig = t->rig, c.vision = t->vision, c.st = t->st;
  c.kp = (const vieo_keypoint*)(W + t->w_kcat), c.desc = W + t->w_dcat, c.uright = (const float*)(Q + t->q_ur);  // mvKeys order
  c.cnt = t->rig ? dO->fcnt : dO->cnt, c.cam_first = dO->cam_first, c.bounds = &t->K.bounds[0][0];
  // one query per (last-frame key, camera) of a rig: most project outside their camera -- the search walks the compacted ones
  c.q1 = (const vieo_proj_query*)(W + t->w_q1c), c.nq1 = t->rig ? dO->nq + 1 : dH->npts + 1, c.q1_cap = kc * nc;
  c.same_point = t->rig ? (const vieo_last_frame_point*)(t->d_up + t->o_pts) : nullptr;
  c.query_src = t->rig ? (const int32_t*)(W + t->w_qsrc) : nullptr;
  c.q2 = (vieo_proj_query*)(W + t->w_q2), c.nq2 = dO->nq, c.q2_cap = t->ccap * nc;
  c.assign = (int32_t*)(W + t->w_assign), c.taken = W + t->w_taken, c.held = W + t->w_held, c.mpref = (int32_t*)(Q + t->q_mpref);
  c.obs = (vieo_pose_obs*)(W + t->w_obs), c.obskey = (int32_t*)(W + t->w_obskey), c.outl = W + t->w_outl, c.key_outlier = Q + t->q_outl;
  c.xyz = (float*)(W + t->w_xyz), c.dep = (float*)(W + t->w_dep), c.consts = dH->consts;
  // (vision only: the leading vieo_pose_frame / vieo_pose_result of the same records)
  c.f1 = &dH->f1, c.f2 = &dH->f2, c.r1 = &dO->r1, c.r2 = &dO->r2, c.fstride = sizeof(vieo_vio_frame);
  c.nm1 = dO->nm, c.nm2 = dO->nm + 1, c.nobs2 = &dO->nobs2[0];
  c.nn_last = t->P.nn_last, c.nn_local = t->P.nn_local, c.close = std::max(10.0f, t->P.th_depth);
  return c;
}

// the refusals, then what the call is going to do (an unwanted pending prefetch is waited for and dropped); nothing is
// written to the pinned blocks or launched here
static int track_check(TrackCall& c) {
  vieo_tracker* t = c.t;
  const vieo_track_input* in = c.in;
  if (!track_input_ok(*in, t->P.width)) return VIEO_E_INVALID;
  for (int i = 0; i < 4; i++) c.imgs[i] = t->rig ? in->images[i] : i == 0 ? in->left : i == 1 ? in->right : nullptr;
  if (!in->use_prefetched)  // (a prefetched frame's images are not read: vieo_hot.h says they may be null then)
    for (int i = 0; i < t->n_img; i++)
      if (!c.imgs[i]) {
        set_error("vieo_track_frame: image %d is null (only a call with use_prefetched = 1 may leave the images out)", i);
        return VIEO_E_INVALID;
      }
  c.t_enter = std::chrono::steady_clock::now();
  if (!track_input_fits(*in, t->kc, t->ccap, t->imu_cap)) {
    set_error("vieo_track_frame: %d last-frame points / %d local points / %d IMU samples exceed the capacities %d / %d / %d",
              in->n_last, in->n_local, in->n_imu, t->kc, t->ccap, t->imu_cap);
    return VIEO_E_CAPACITY;
  }
  const int rc = require_device();
  if (rc != VIEO_OK) return rc;
  c.nl = in->n_last, c.nc = in->n_local, c.pref = in->use_prefetched != 0;
  if (c.pref && !t->pref_valid) {
    set_error("vieo_track_frame: use_prefetched without a pending prefetch (the previous call carried no next_left / next_right)");
    return VIEO_E_INVALID;
  }
  // the next frame's images: next_left / next_right (rectified pair) or next_images[c] (rig)
  for (int i = 0; i < 4; i++) c.nx[i] = t->rig ? in->next_images[i] : i == 0 ? in->next_left : i == 1 ? in->next_right : nullptr;
  for (int i = 0; i < t->n_img; i++) c.n_next += c.nx[i] != nullptr;
  if (c.n_next != 0 && c.n_next != t->n_img) {
    set_error("vieo_track_frame: the next frame's images come complete (%d of %d given)", c.n_next, t->n_img);
    return VIEO_E_INVALID;
  }
  if (!c.pref && t->pref_valid) {  // a pending prefetch the caller does not want: let it finish, forget it
    (void)hipStreamSynchronize(t->st_pref);
    t->pref_valid = false;
  }
  c.new_local = track_local_changed(*in, t->local_version, t->n_local_dev);
  if (c.new_local && (!in->local_points || !in->local_desc)) return VIEO_E_INVALID;
  const bool spec_any = !t->vision && in->next_imu && in->next_n_imu > 0 && in->next_n_imu <= t->imu_cap;
  c.spec_ref = spec_any && in->next_ref_bias != nullptr, c.spec = spec_any && !c.spec_ref;
  c.H = (TrkHdr*)(t->h_up + t->o_hdr), c.dH = (TrkHdr*)(t->d_up + t->o_hdr);
  c.dO = (TrkOut*)(t->d_out + t->q_hdr), c.O = (const TrkOut*)(t->h_out + t->q_hdr);
  c.d_kp = (vieo_keypoint*)(t->d_work + t->w_kp), c.d_desc = t->d_work + t->w_desc;
  // (a frame extracted ahead has no extraction to run beside: prediction and projection stay on the main stream, without
  // the two event hops to the second one and back: ~12 us)
  c.s_head = c.pref ? t->st : t->st_imu;
  c.chain = track_chain_of(t, c.dH, c.dO);
  return VIEO_OK;
}

// the pinned blocks: header, IMU samples, images, the last frame's points; the local map when it changed
static void track_fill_upload(TrackCall& c) {
  vieo_tracker* t = c.t;
  const vieo_track_input* in = c.in;
  const int nl = c.nl, nc = c.nc, W = t->P.width, Hh = t->P.height;
  TrkHdr& H = *c.H;
  H.cam.th = t->P.th_last;
  H.nav_ref = in->nav_ref, H.nav_last = in->nav_last;
  track_fill_problem(H.f1, *in), track_fill_problem(H.f2, *in);
  H.ti = in->t_ref, H.tj = in->t_cur;
  for (int k = 0; k < 3; k++) H.bg[k] = in->nav_ref.bg[k], H.ba[k] = in->nav_ref.ba[k];
  H.first[0] = 0, H.first[1] = in->n_imu, H.npts[0] = nl, H.npts[1] = nl * t->nc;
  if (in->n_imu) memcpy(t->h_up + t->o_imu, in->imu, (size_t)in->n_imu * sizeof(vieo_imu_sample));
  for (int i = 0; i < (c.pref ? 0 : t->n_img); i++) track_copy_plane(t->h_up + t->o_img + (size_t)i * W * Hh, c.imgs[i], W, Hh, in->stride);
  if (nl) {
    memcpy(t->h_up + t->o_pts, in->last_points, (size_t)nl * sizeof(vieo_last_frame_point));
    track_pack_xyz((float*)(t->h_up + t->o_xyz), in->last_points, nl);
    memcpy(t->h_up + t->o_dep, in->last_track_depth, (size_t)nl * 4);
  }
  if (nc) memcpy(t->h_up + t->o_alias, in->local_alias, (size_t)nc * 4);
  if (c.new_local) {
    memcpy(t->h_loc + t->l_cpt, in->local_points, (size_t)nc * sizeof(vieo_frustum_point));
    memcpy(t->h_loc + t->l_cdesc, in->local_desc, (size_t)nc * 32);
    track_pack_xyz((float*)(t->h_loc + t->l_xyz), in->local_points, nc);
  }
}

// ExtractORB of n_img images on the extractor's stream and, for rectified pairs, ComputeStereoMatches
static int track_extract(vieo_tracker* t, const uint8_t* d_img, vieo_keypoint* kp, uint8_t* desc, int32_t* cnt, bool stereo, float* ur,
                         float* dp) {
  const int W = t->P.width, Hh = t->P.height;
  const int* lapping = t->rig && t->R.use_lapping ? t->R.lapping : nullptr;
  int rc = vieo_orb_extract_batch_device(t->ext, d_img, t->n_img, W, Hh, W, (size_t)W * Hh, lapping, kp, desc, t->cap, cnt);
  if (rc == VIEO_OK && stereo)
    rc = vieo_stereo_match_rectified_batch_device(t->ext, 1, kp, desc, cnt, t->cap, t->P.baseline, t->P.bf, ur, dp);
  return rc;
}

// One copy up; then the frame's keys and descriptors: extracted here, or adopted from the slot the third stream
// extracted into beside the previous call's tail.
static int track_head(TrackCall& c) {
  vieo_tracker* t = c.t;
  hipStream_t st = t->st;
  const int cap = t->cap;
  VIEO_HIP_CHECK(hipEventRecord(t->ev_t0, st));
  VIEO_HIP_CHECK(hipMemcpyAsync(t->d_up, t->h_up, t->up_fixed + (size_t)c.nc * 4, hipMemcpyHostToDevice, st));
  VIEO_HIP_CHECK(hipEventRecord(t->ev_up, st));
  if (!c.pref) {
    VIEO_HIP_CHECK(hipMemcpyAsync(t->d_up + t->o_img, t->h_up + t->o_img, t->img_bytes, hipMemcpyHostToDevice, st));
    return track_extract(t, t->d_up + t->o_img, c.d_kp, c.d_desc, c.dO->cnt, false, nullptr, nullptr);
  }
  VIEO_HIP_CHECK(hipStreamWaitEvent(st, t->ev_pref, 0));
  const int n_kp16 = (int)(((size_t)t->n_img * cap * sizeof(vieo_keypoint) + 15) / 16), n_desc16 = t->n_img * cap * 2;
  const int n_f16 = t->rig ? 0 : (cap + 3) / 4;  // (a rig frame's stereo stage runs in the call: it fills mvKeys-order tables)
  hipLaunchKernelGGL(k_track_adopt, dim3(32), dim3(256), 0, st, (const uint4*)(t->d_slot + t->s_kp), (uint4*)c.d_kp, n_kp16,
                     (const uint4*)(t->d_slot + t->s_desc), (uint4*)c.d_desc, n_desc16, (const uint4*)(t->d_slot + t->s_ur),
                     (uint4*)(t->d_out + t->q_ur), (const uint4*)(t->d_slot + t->s_dp), (uint4*)(t->d_out + t->q_dp), n_f16,
                     (const int32_t*)(t->d_slot + t->s_cnt), c.dO->cnt, 2 * t->n_img);
  t->pref_valid = false;
  return VIEO_OK;
}

// the first search's queries from the predicted pose: SearchByProjection's projection of the last frame's points and, for
// rigs, the compaction of the valid (point, camera) pairs
static int track_project(vieo_tracker* t, hipStream_t s) {
  const int kc = t->kc, nc = t->nc;
  TrkHdr* dH = (TrkHdr*)(t->d_up + t->o_hdr);
  uint8_t* W = t->d_work;
  vieo_proj_query* d_q1 = (vieo_proj_query*)(W + t->w_q1);
  const vieo_last_frame_point* d_pts = (const vieo_last_frame_point*)(t->d_up + t->o_pts);
  if (!t->rig) return vieo_sbp_project_last_frame_batch_device(d_pts, dH->npts, kc, 1, &dH->cam, d_q1, s);
  const int rc = vieo_sbp_project_last_frame_rig_batch_device(d_pts, dH->npts, kc, 1, &dH->cam, (const vieo_sbp_rig*)t->d_const,
                                                              nc, d_q1, s);
  if (rc != VIEO_OK) return rc;
  return vieo_track_compact_queries_batch_device(d_q1, dH->npts + 1, kc * nc, 1, (vieo_proj_query*)(W + t->w_q1c),
                                                 (int32_t*)(W + t->w_qsrc), ((TrkOut*)(t->d_out + t->q_hdr))->nq + 1, s);
}

// ComputeStereoFishEyeMatches (Frame.cc:613-779) into mvKeys order.  What tracking reads of it -- the concatenated keys and
// descriptors, the cameras' ranges, uright = -1 -- does not depend on the matches: that part (VIEO_FISHEYE_CONCAT) stays on
// the main stream; the matches / groups / depths (VIEO_FISHEYE_GROUPS: 0.3 ms of a 4-camera frame), outputs of the frame
// only, run on the second stream beside the searches and optimisations and are joined before the copy back.
static int track_fisheye_part(TrackCall& c, int part, hipStream_t s) {
  vieo_tracker* t = c.t;
  uint8_t *Wk = t->d_work, *Q = t->d_out;
  TrkOut* dO = c.dO;
  return vieo_stereo_fisheye_match_batch_device_part(
      t->fe, c.d_kp, c.d_desc, dO->cnt, 1, (vieo_keypoint*)(Wk + t->w_kcat), Wk + t->w_dcat, dO->cam_first, dO->fcnt,
      (float*)(Q + t->q_dp), (float*)(Q + t->q_ur), (int32_t*)(Q + t->q_kg), (int32_t*)(Q + t->q_gidx), Q + t->q_good,
      (double*)(Q + t->q_p3d), dO->fe_hdr, part, s);
}

// PredictNavStateByIMU and the projection of the last frame's points need nothing of the new images: second stream, beside
// the extraction, handed over AFTER the extraction's launches (the head of the critical path).  The pre-integration in front
// runs here, or was run ahead by the previous call (next_imu) if what it integrated is bit for bit what this call asks for.
static int track_predict_and_stereo(TrackCall& c) {
  vieo_tracker* t = c.t;
  const vieo_track_input* in = c.in;
  uint8_t* Wk = t->d_work;
  TrkHdr* dH = c.dH;
  hipStream_t s_head = c.s_head;
  const TrkTables tables{(const float*)(t->d_up + t->o_xyz), (const float*)(t->d_up + t->o_dep), (float*)(Wk + t->w_xyz),
                         (float*)(Wk + t->w_dep)};
  int rc;
  if (!c.pref) VIEO_HIP_CHECK(hipStreamWaitEvent(t->st_imu, t->ev_up, 0));
  if (!t->vision) {
    const bool ahead = t->spec_valid && in->n_imu == t->spec_n && in->t_ref == t->spec_ti && in->t_cur == t->spec_tj &&
                       (in->n_imu == 0 || memcmp(in->imu, t->spec_samples.data(), (size_t)in->n_imu * sizeof(vieo_imu_sample)) == 0) &&
                       memcmp(in->nav_ref.bg, t->spec_bias, 24) == 0 && memcmp(in->nav_ref.ba, t->spec_bias + 3, 24) == 0;
    t->spec_valid = false;
    const uint8_t *pre_at = ahead ? t->d_spec + t->sp_pre : Wk + t->w_pre, *prv_at = ahead ? t->d_spec + t->sp_prv : Wk + t->w_prv;
    const uint8_t* pst_at = ahead ? t->d_spec + t->sp_pst : Wk + t->w_pst;
    if (ahead) {
      t->spec_used++;
      // (it ran on the second stream -- which vieo_tracker_reprobe may have replaced since: wait for it by its event either way)
      VIEO_HIP_CHECK(hipStreamWaitEvent(s_head, t->ev_spec, 0));
    } else if ((rc = vieo_imu_preintegrate_batch_device(&dH->noise, (const vieo_imu_sample*)(t->d_up + t->o_imu), dH->first, &dH->ti,
                                                        &dH->tj, dH->bg, dH->ba, 1, (vieo_imu_preint*)(Wk + t->w_pre),
                                                        (double*)(Wk + t->w_prv), (int32_t*)(Wk + t->w_pst), s_head)) != VIEO_OK)
      return rc;
    hipLaunchKernelGGL(k_track_predict, dim3(1 + kTableBlocks), dim3(64), 0, s_head, dH, c.dO, (const vieo_imu_preint*)pre_at,
                       (const double*)prv_at, (const int32_t*)pst_at, (double*)(t->d_spec + t->sp_bias), tables);
  } else {
    hipLaunchKernelGGL(k_track_set_pose, dim3(1 + kTableBlocks), dim3(64), 0, s_head, dH, c.dO, tables);
  }
  VIEO_HIP_CHECK(hipGetLastError());
  if ((rc = track_project(t, s_head)) != VIEO_OK) return rc;
  if (!c.pref) VIEO_HIP_CHECK(hipEventRecord(t->ev_imu, t->st_imu));  // what the first search waits for
  // the stereo stage on the main stream (a prefetched pair's ran with its extraction)
  if (t->rig)
    rc = track_fisheye_part(c, VIEO_FISHEYE_CONCAT, t->st);
  else if (!c.pref)
    rc = vieo_stereo_match_rectified_batch_device(t->ext, 1, c.d_kp, c.d_desc, c.dO->cnt, t->cap, t->P.baseline, t->P.bf,
                                                  (float*)(t->d_out + t->q_ur), (float*)(t->d_out + t->q_dp));
  if (rc != VIEO_OK) return rc;
  VIEO_HIP_CHECK(hipEventRecord(t->ev_head, t->st));  // the extractor's pyramids and scratch are free from here on
  VIEO_HIP_CHECK(hipEventRecord(t->ev_ext, t->st));   // mvKeys / mDescriptors are final: what the second stream reads of this one
  return VIEO_OK;
}

// The next frame's pre-integration run ahead (second stream): samples and [t_ref, next_t_cur] go up (ref_bias: a named reference's) ...
static int spec_upload(vieo_tracker* t, const vieo_track_input* in, double t_ref, const double* ref_bias) {
  SpecImu& S = *(SpecImu*)t->h_spec;
  S.noise = t->P.noise, S.ti = t_ref, S.tj = in->next_t_cur, S.first[0] = 0, S.first[1] = in->next_n_imu;
  if (ref_bias) memcpy(S.xbias, ref_bias, sizeof(S.xbias));
  memcpy(t->h_spec + t->sp_samples, in->next_imu, (size_t)in->next_n_imu * sizeof(vieo_imu_sample));
  VIEO_HIP_CHECK(hipMemcpyAsync(t->d_spec, t->h_spec, t->sp_samples + (size_t)in->next_n_imu * sizeof(vieo_imu_sample),
                                hipMemcpyHostToDevice, t->st_imu));
  return VIEO_OK;
}
// ... and PreIntegration runs over them with the bias at `bias` in HBM.  What was integrated is kept: the next call compares.
static int spec_integrate(vieo_tracker* t, const vieo_track_input* in, double t_ref, const double* bias) {
  SpecImu* dS = (SpecImu*)t->d_spec;
  const int rc = vieo_imu_preintegrate_batch_device(&dS->noise, (const vieo_imu_sample*)(t->d_spec + t->sp_samples), dS->first, &dS->ti,
                                                    &dS->tj, bias, bias + 3, 1, (vieo_imu_preint*)(t->d_spec + t->sp_pre),
                                                    (double*)(t->d_spec + t->sp_prv), (int32_t*)(t->d_spec + t->sp_pst), t->st_imu);
  if (rc != VIEO_OK) return rc;
  VIEO_HIP_CHECK(hipEventRecord(t->ev_spec, t->st_imu));
  t->spec_samples.assign(in->next_imu, in->next_imu + in->next_n_imu);
  t->spec_n = in->next_n_imu, t->spec_ti = t_ref, t->spec_tj = in->next_t_cur;
  return VIEO_OK;
}

// The rest of the second stream's work is read by the chain behind the first optimisation at the earliest: the host hands
// it over AFTER that kernel's launch, where it gets ahead of the device again.
static int track_side_rest(TrackCall& c) {
  vieo_tracker* t = c.t;
  const vieo_track_input* in = c.in;
  uint8_t* Wk = t->d_work;
  hipStream_t sb = t->st_imu;
  const int kc = t->kc, nc = c.nc;
  const double* bj_bar = (const double*)(t->d_spec + t->sp_bias);  // k_track_predict left it there
  int rc;
  if (c.new_local) {  // a changed local map; nothing before the local-map queries reads it
    VIEO_HIP_CHECK(hipMemcpyAsync(t->d_loc + t->l_cpt, t->h_loc + t->l_cpt, (size_t)nc * sizeof(vieo_frustum_point),
                                  hipMemcpyHostToDevice, sb));
    VIEO_HIP_CHECK(hipMemcpyAsync(t->d_loc + t->l_cdesc, t->h_loc + t->l_cdesc, (size_t)nc * 32, hipMemcpyHostToDevice, sb));
    VIEO_HIP_CHECK(hipMemcpyAsync(Wk + t->w_xyz + (size_t)kc * 12, t->h_loc + t->l_xyz, (size_t)nc * 12, hipMemcpyHostToDevice, sb));
    t->local_version = in->local_version, t->n_local_dev = nc;
    VIEO_HIP_CHECK(hipEventRecord(t->ev_tab, sb));  // (joined below)
  }
  VIEO_HIP_CHECK(hipStreamWaitEvent(sb, t->ev_ext, 0));
  if (t->rig) {
    if ((rc = track_fisheye_part(c, VIEO_FISHEYE_GROUPS, sb)) != VIEO_OK) return rc;
    VIEO_HIP_CHECK(hipEventRecord(t->ev_fe, sb));
  }
  // this frame as the reference: the samples go up ahead of the keys' / descriptors' copies back, the integration behind them
  if (c.spec && (rc = spec_upload(t, in, in->t_cur, nullptr)) != VIEO_OK) return rc;
  VIEO_HIP_CHECK(hipMemcpyAsync(t->h_out + t->q_kp, Wk + t->w_kcat, (size_t)kc * sizeof(vieo_keypoint), hipMemcpyDeviceToHost, sb));
  VIEO_HIP_CHECK(hipMemcpyAsync(t->h_out + t->q_desc, Wk + t->w_dcat, (size_t)kc * 32, hipMemcpyDeviceToHost, sb));
  VIEO_HIP_CHECK(hipEventRecord(t->ev_kd, sb));
  if (c.spec && (rc = spec_integrate(t, in, in->t_cur, bj_bar)) != VIEO_OK) return rc;
  // a reference the caller names: both steps here (starting them behind the prediction was measured and dropped)
  if (c.spec_ref && ((rc = spec_upload(t, in, in->next_t_ref, in->next_ref_bias)) != VIEO_OK ||
                     (rc = spec_integrate(t, in, in->next_t_ref, ((SpecImu*)t->d_spec)->xbias)) != VIEO_OK))
    return rc;
  if (c.new_local) VIEO_HIP_CHECK(hipStreamWaitEvent(t->st, t->ev_tab, 0));  // the main stream: the changed local map is in place
  return VIEO_OK;
}

// The chain behind the prediction, the copies back, the end of the GPU time.  first: the call's first run -- the first search's
// queries were made beside the extraction (joined here), the second stream gets its rest; a repeat projects again and waits.
static int track_tail(TrackCall& c, bool first) {
  vieo_tracker* t = c.t;
  const TrackChain& ch = c.chain;
  hipStream_t st = t->st;
  if (first && !c.pref) VIEO_HIP_CHECK(hipStreamWaitEvent(st, t->ev_imu, 0));
  const int rc = track_run_chain(
      ch, first, [&] { return track_project(t, st); }, [&] { return first ? track_side_rest(c) : (int)VIEO_OK; },
      [&] {  // (the kernel reads only the leading vieo_pose_frame / vieo_pose_result of its two arguments)
        return vieo_track_local_queries_device(&t->K.ff, (const vieo_vio_frame*)ch.f1, (const vieo_vio_result*)ch.r1,
                                               (const vieo_frustum_point*)(t->d_loc + t->l_cpt), t->d_loc + t->l_cdesc,
                                               (const int32_t*)(t->d_up + t->o_alias), ch.held, ch.pcap, c.nc, t->P.th_local,
                                               t->rig ? t->R.th_far_pts : 0.f, ch.consts + 16, ch.q2, ch.dep + ch.kc, ch.nq2, st);
      });
  if (rc != VIEO_OK) return rc;
  // results: [header | uright | depth | point_ref | outlier | (rig: key -> group, the groups)] and the candidates' depths
  if (t->rig) VIEO_HIP_CHECK(hipStreamWaitEvent(st, t->ev_fe, 0));  // the stereo groups of the frame (second stream)
  VIEO_HIP_CHECK(hipMemcpyAsync(t->h_out, t->d_out, t->q_small_end, hipMemcpyDeviceToHost, st));
  if (c.nc > 0) VIEO_HIP_CHECK(hipMemcpyAsync(t->h_out + t->q_cdep, ch.dep + ch.kc, (size_t)c.nc * 4, hipMemcpyDeviceToHost, st));
  if (first) VIEO_HIP_CHECK(hipStreamWaitEvent(st, t->ev_kd, 0));  // (the keys' / descriptors' copies)
  VIEO_HIP_CHECK(hipEventRecord(t->ev_t1, st));
  if (!first) VIEO_HIP_CHECK(hipStreamSynchronize(st));
  return VIEO_OK;
}

// The NEXT frame's Frame::Frame on the third stream, beside this frame's searches and optimisations (queued by now), into
// the slot the next call adopts; then the ONE host synchronisation of the frame.
static int track_prefetch_next_and_wait(TrackCall& c) {
  vieo_tracker* t = c.t;
  hipStream_t sp = t->st_pref;
  if (c.n_next) {
    // (the previous prefetch's copy up left these planes long ago, but nothing in the stream order says so: ask)
    if (t->h2d_pending) VIEO_HIP_CHECK(hipEventSynchronize(t->ev_h2d));
    for (int i = 0; i < t->n_img; i++)
      track_copy_plane(t->h_next + i * (t->img_bytes / t->n_img), c.nx[i], t->P.width, t->P.height, c.in->stride);
    VIEO_HIP_CHECK(hipStreamWaitEvent(sp, t->ev_head, 0));
    VIEO_HIP_CHECK(hipMemcpyAsync(t->d_next, t->h_next, t->img_bytes, hipMemcpyHostToDevice, sp));
    VIEO_HIP_CHECK(hipEventRecord(t->ev_h2d, sp));
    t->h2d_pending = true;
    hipStream_t keep = t->ext->stream;
    t->ext->stream = sp;  // (the extractor and the stereo matcher launch on the handle's stream)
    const int rc = track_extract(t, t->d_next, (vieo_keypoint*)(t->d_slot + t->s_kp), t->d_slot + t->s_desc,
                                 (int32_t*)(t->d_slot + t->s_cnt),
                                 !t->rig, (float*)(t->d_slot + t->s_ur), (float*)(t->d_slot + t->s_dp));
    t->ext->stream = keep;
    if (rc != VIEO_OK) {
      (void)hipStreamSynchronize(sp);
      return rc;
    }
    VIEO_HIP_CHECK(hipEventRecord(t->ev_pref, sp));
    t->pref_valid = true, t->pref_frames++;
  }
  VIEO_HIP_CHECK(hipStreamSynchronize(t->st));
  return VIEO_OK;
}

// The repeats of the chain.  Tracking.cc:301-309 / :1869-1876: the wider window -- only the search threshold changes, all
// before the projection is still in HBM.  Rigs: a replica of an optimisation never became resident (vieo_pose_set_replicas
// in include/vieo_hot.h: the device is shared) -- again with one workgroup per optimisation; the frame is late, not lost.
static int track_repeats(TrackCall& c) {
  vieo_tracker* t = c.t;
  int rc = VIEO_OK;
  if (track_wants_wider_window(track_pre_ok(t->vision, c.O->preint_status[0], c.O->imu.dt), c.O->nm[0])) {
    c.widened = 1;
    const float th2 = 2 * t->P.th_last;
    VIEO_HIP_CHECK(hipMemcpyAsync(&c.dH->cam.th, &th2, 4, hipMemcpyHostToDevice, t->st));
    rc = track_tail(c, false);
  }
  if (rc == VIEO_OK && t->rig && (c.O->r1.base.status == VIEO_E_HIP || c.O->r2.base.status == VIEO_E_HIP)) {
    const int was = vieo_pose_set_replicas(0);
    rc = track_tail(c, false);
    (void)vieo_pose_set_replicas(was);
    if (rc == VIEO_OK) t->replica_repeats++;
  }
  return rc;
}

// the frame's outputs; what the next call's run-ahead comparison needs; the watch over the chain's GPU time
static void track_output(TrackCall& c) {
  vieo_tracker* t = c.t;
  vieo_track_output* out = c.out;
  const TrkOut* O = c.O;
  const uint8_t* Q = t->h_out;
  if (c.spec || c.spec_ref) {  // (the bias the run-ahead integration used: the next call's nav_ref must carry exactly it)
    for (int k = 0; k < 3; k++) t->spec_bias[k] = O->nav_pred.bg[k], t->spec_bias[3 + k] = O->nav_pred.ba[k];
    if (c.spec_ref) memcpy(t->spec_bias, c.in->next_ref_bias, sizeof(t->spec_bias));
    t->spec_valid = true;
  }
  float ms_gpu = 0;
  (void)hipEventElapsedTime(&ms_gpu, t->ev_t0, t->ev_t1);
  const float ms_host = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - c.t_enter).count();
  track_fill_output(out, t->vision, O->preint_status[0], O->nm[0], O->nm[1], c.widened, O->nav_pred, &O->imu, &O->r1, &O->r2,
                    sizeof(vieo_vio_result), ms_gpu, ms_host);
  if (t->rig) {
    out->n_keys = std::min(O->cam_first[t->nc], t->kc);
    for (int i = 0; i <= t->nc; i++) out->cam_first[i] = O->cam_first[i];
    for (int i = 0; i < t->nc; i++) out->mono_index[i] = O->cnt[2 * i + 1];
    out->stereo_status = O->fe_hdr[3], out->n_groups = O->fe_hdr[3] ? 0 : O->fe_hdr[0], out->n_stereo_matches = O->fe_hdr[1];
    out->key_group = (const int32_t*)(Q + t->q_kg), out->group_idx = (const int32_t*)(Q + t->q_gidx);
    out->group_good = Q + t->q_good, out->group_p3d = (const double*)(Q + t->q_p3d);
  } else {
    out->n_keys = std::min(O->cnt[0], t->cap);
    out->cam_first[1] = out->n_keys;
  }
  out->key_cap = t->kc, out->keys = (const vieo_keypoint*)(Q + t->q_kp), out->desc = Q + t->q_desc;
  out->uright = (const float*)(Q + t->q_ur), out->depth = (const float*)(Q + t->q_dp),
      out->local_track_depth = (const float*)(Q + t->q_cdep);
  out->point_ref = (const int32_t*)(Q + t->q_mpref), out->outlier = Q + t->q_outl;
  // eight frames in a row 30 % above the running median GPU time -> look at the second stream again (at most once per 64 frames)
  const float med = track_gpu_median(t, 16);
  t->slow_run = (med > 0 && ms_gpu > 1.3f * med && !c.widened) ? t->slow_run + 1 : 0;
  t->gpu_ring[t->gpu_n % 32] = ms_gpu, t->gpu_n++, t->frames_since_check++;
  // (not while a prefetch is in flight: the probe's spin kernels would share the device with it and skew the ratio)
  if (t->slow_run >= 8 && t->frames_since_check >= 64 && !t->pref_valid) {
    (void)vieo_tracker_reprobe(t);
    t->frames_since_check = 0, t->slow_run = 0, t->gpu_n = 0;
  }
}

// an error in the middle: work queued on the streams still reads the pinned blocks, which the next call would overwrite -- wait
static int track_fail(vieo_tracker* t, int rc) {
  if (t->st_pref) (void)hipStreamSynchronize(t->st_pref), t->pref_valid = false;
  t->spec_valid = false;
  (void)hipStreamSynchronize(t->st_imu);
  (void)hipStreamSynchronize(t->st);
  return rc;
}

extern "C" {

int vieo_track_frame(vieo_tracker* t, const vieo_track_input* in, vieo_track_output* out) {
  if (!t || !in || !out) return VIEO_E_INVALID;
  TrackCall c{t, in, out};
  int rc = track_check(c);
  if (rc != VIEO_OK) return rc;
  track_fill_upload(c);
  // the launches, in stream order; a failure waits for what is queued (track_fail)
  if ((rc = track_head(c)) != VIEO_OK || (rc = track_predict_and_stereo(c)) != VIEO_OK ||
      (rc = track_tail(c, true)) != VIEO_OK || (rc = track_prefetch_next_and_wait(c)) != VIEO_OK ||
      (rc = track_repeats(c)) != VIEO_OK)
    return track_fail(t, rc);
  track_output(c);
  return VIEO_OK;
}

}  // extern "C"
