// tracker_multi.hip -- one frame of each of n live sequences as ONE call (vieo_track_frames).
//
// vieo_track_frame's chain (tracker.hip) with every one-frame launch replaced by one launch over the call's n frames; the
// per-frame inputs, the optimiser problems and the results are structure-of-arrays blocks that the batched entries read
// as they are:
//
//   H2D (one block: headers [n], IMU samples, last frames' points [n][key_cap], aliases [n][ccap]; the slots' image planes)
//   stream B:  changed local maps -> slot tables [slot][ccap];  k_imu_preint over n intervals;  k_track_predict_multi
//              (PredictNavStateByIMU per frame + the point tables [n][pcap]);  sbp_project [n]
//   stream A:  extract x 2n -> stereo [n]
//              search(last frame) [n] -> merge + build_obs [n] -> PoseOptimization [n] -> after_pose + held [n]
//              -> local queries through the slots [n] -> search(local map) [n] -> merge + build_obs [n]
//              -> PoseOptimization(bComputeMarg) [n] -> k_track_finish [n]
//   D2H, ONE host synchronisation (+ the chain again over all n frames when one of them takes the wider window).
//
// The chain on stream A behind the stereo stage is track_run_chain (track_chain.h), the function vieo_track_frame runs
// with n = 1; the constants, the record filling, the checks and the decisions are that header's too.
//
// Every stage computes a frame from that frame's data alone, in fixed orders (no floating-point atomics): a frame's bytes
// do not depend on the batch it is in, and equal what vieo_track_frame gives for it.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "orb_internal.h"
#include "track_chain.h"

namespace vieo {

// one call's point-table copies (k_track_predict_multi / k_track_set_pose_multi, blocks 1..kTableBlocks of frame i):
// the last frame's xyz / track depth from the upload block and the slot's local-map xyz into the frame's tables
struct MultiTables {
  const float *last_xyz, *last_dep;  // [n][kc * 3], [n][kc]
  const float* loc_xyz;              // [slot][ccap * 3]
  float *xyz_out, *dep_out;          // [n][pcap * 3], [n][pcap]
  const int32_t *n_last, *n_local, *slot;
  int kc, ccap, pcap;
};
__device__ __forceinline__ void multi_fill_tables(const MultiTables& T, int i) {
  const TrkTables t{T.last_xyz + (size_t)i * T.kc * 3, T.last_dep + (size_t)i * T.kc, T.xyz_out + (size_t)i * T.pcap * 3,
                    T.dep_out + (size_t)i * T.pcap};
  track_fill_tables(t, T.n_last[i]);
  const float* src = T.loc_xyz + (size_t)T.slot[i] * T.ccap * 3;
  float* dst = T.xyz_out + ((size_t)i * T.pcap + T.kc) * 3;
  const int i0 = (blockIdx.x - 1) * 64 + threadIdx.x, step = kTableBlocks * 64, nl = 3 * T.n_local[i];
  for (int j = i0; j < nl; j += step) dst[j] = src[j];
}

// grid (1 + kTableBlocks, n): workgroup 0 of frame i is k_track_predict's body for that frame
__global__ void __launch_bounds__(64)
k_track_predict_multi(const vieo_navstate* __restrict__ nav_ref, const vieo_navstate* __restrict__ nav_last,
                      vieo_vio_frame* __restrict__ f1, vieo_vio_frame* __restrict__ f2, vieo_sbp_camera* __restrict__ cam,
                      vieo_navstate* __restrict__ nav_pred, vieo_imu_preint* __restrict__ imu_out, double* __restrict__ sigma_out,
                      int32_t* __restrict__ status_out, const vieo_imu_preint* __restrict__ pre,
                      const double* __restrict__ sigma_prv, const int32_t* __restrict__ status, double* __restrict__ next_bias,
                      MultiTables tables) {
  const int i = blockIdx.y;
  if (blockIdx.x > 0) return multi_fill_tables(tables, i);
  __shared__ vieo_navstate s_nav;
  track_predict_frame(nav_ref + i, nav_last + i, f1 + i, f2 + i, cam + i, nav_pred + i, imu_out + i, sigma_out + (size_t)i * 81,
                      status_out + i, pre + i, sigma_prv + (size_t)i * 81, status + i, next_bias + (size_t)i * 6, s_nav);
}

// the vision-only form: k_track_set_pose's body per frame, the optimiser problems are vieo_pose_frame records
__global__ void __launch_bounds__(64)
k_track_set_pose_multi(const vieo_navstate* __restrict__ nav_ref, const vieo_navstate* __restrict__ nav_last,
                       vieo_pose_frame* __restrict__ f1, vieo_pose_frame* __restrict__ f2, vieo_sbp_camera* __restrict__ cam,
                       vieo_navstate* __restrict__ nav_pred, int32_t* __restrict__ status_out, MultiTables tables) {
  const int i = blockIdx.y;
  if (blockIdx.x > 0) return multi_fill_tables(tables, i);
  track_set_pose_frame(nav_ref + i, nav_last + i, f1[i].Rcb, f1[i].tcb, cam + i, &f1[i].nav, &f2[i].nav, nav_pred + i,
                       status_out + i);
}

// Where one call's arrays sit in the upload and download blocks: packed for its n frames, so that each block travels
// as one copy of its used prefix.
struct MultiLayout {
  size_t u_cam, u_f1, u_f2, u_nref, u_nlast, u_ti, u_tj, u_bg, u_ba, u_first, u_nl, u_nloc, u_slot, u_pts, u_xyz, u_dep,
      u_alias, u_imu;
  size_t q_cnt, q_nm1, q_nm2, q_nq2, q_pst, q_nobs, q_r1, q_r2, q_nav, q_imu, q_sig, q_ur, q_dp, q_mpref, q_outl, q_small,
      q_kp, q_desc, q_cdep, q_end;
};

}  // namespace vieo

using namespace vieo;

struct vieo_tracker_multi {
  vieo_tracker_params P;
  bool vision = false;
  int max_seq = 0;
  vieo_orb* ext = nullptr;
  hipStream_t st = nullptr, st_imu = nullptr;
  hipEvent_t ev_up = nullptr, ev_imu = nullptr, ev_ext = nullptr, ev_kd = nullptr, ev_t0 = nullptr, ev_t1 = nullptr;
  float side_ratio = 0.f;
  int cap = 0, kc = 0, ccap = 0, pcap = 0, imu_cap = 512;
  size_t fstride = 0, rstride = 0;  // optimiser problem / result records: vieo_vio_* or vieo_pose_* (vision-only)
  TrackConstants K;  // cam0 / f1_0 / f2_0: the constant parts of a frame's records; the frustum frame, the bounds
  std::vector<int> local_version, n_local_dev;  // per slot: what its device table holds (vieo_tracker's pair)
  size_t npx = 0;
  // pinned blocks and their device twins
  uint8_t *h_up = nullptr, *d_up = nullptr;    // per-call upload (MultiLayout u_*)
  uint8_t *h_img = nullptr, *d_img = nullptr;  // image planes: pinned [slot][2][npx], device [frame][2][npx]
  uint8_t *h_loc = nullptr, *d_loc = nullptr;  // local maps: points [slot][ccap] | descriptors [slot][ccap][32] | xyz [slot][ccap][3]
  uint8_t *h_out = nullptr, *d_out = nullptr;  // per-call download (MultiLayout q_*)
  uint8_t* d_work = nullptr;                   // device-only scratch [max_seq][...]
  uint8_t* d_const = nullptr;                  // vieo_imu_noise | inv_sigma2[16] | scale[16]
  size_t l_pts, l_desc, l_xyz;                 // offsets of the three slot tables in the local block
  size_t c_consts, up_bytes, out_bytes, loc_bytes, work_bytes, const_bytes, img_bytes;
  size_t w_kp, w_desc, w_q1, w_q2, w_assign, w_taken, w_held, w_obs, w_obskey, w_outl, w_xyz, w_dep, w_pre, w_prv, w_pst, w_bias;
};

static MultiLayout multi_layout(const vieo_tracker_multi* m, int n) {
  MultiLayout L;
  const size_t N = n;
  Layout U, Q;
  L.u_cam = U.take(N * sizeof(vieo_sbp_camera)), L.u_f1 = U.take(N * m->fstride), L.u_f2 = U.take(N * m->fstride);
  L.u_nref = U.take(N * sizeof(vieo_navstate)), L.u_nlast = U.take(N * sizeof(vieo_navstate));
  L.u_ti = U.take(N * 8), L.u_tj = U.take(N * 8), L.u_bg = U.take(N * 24), L.u_ba = U.take(N * 24), L.u_first = U.take((N + 1) * 4);
  L.u_nl = U.take(N * 4), L.u_nloc = U.take(N * 4), L.u_slot = U.take(N * 4);
  L.u_pts = U.take(N * m->kc * sizeof(vieo_last_frame_point)), L.u_xyz = U.take(N * m->kc * 12), L.u_dep = U.take(N * m->kc * 4);
  L.u_alias = U.take(N * m->ccap * 4);
  L.u_imu = U.take(N * m->imu_cap * sizeof(vieo_imu_sample));  // (last: a call uploads up to its samples)
  L.q_cnt = Q.take(N * 2 * 8), L.q_nm1 = Q.take(N * 4), L.q_nm2 = Q.take(N * 4), L.q_nq2 = Q.take(N * 4), L.q_pst = Q.take(N * 4);
  L.q_nobs = Q.take(N * 4), L.q_r1 = Q.o, L.q_r2 = Q.o + N * m->rstride, (void)Q.take(2 * N * m->rstride);  // (adjacent: one clear)
  L.q_nav = Q.take(N * sizeof(vieo_navstate)), L.q_imu = Q.take(N * sizeof(vieo_imu_preint)), L.q_sig = Q.take(N * 81 * 8);
  L.q_ur = Q.take(N * m->kc * 4), L.q_dp = Q.take(N * m->kc * 4), L.q_mpref = Q.take(N * m->kc * 4), L.q_outl = Q.take(N * m->kc);
  L.q_small = Q.o;
  L.q_kp = Q.take(N * m->cap * sizeof(vieo_keypoint)), L.q_desc = Q.take(N * m->cap * 32), L.q_cdep = Q.take(N * m->ccap * 4);
  L.q_end = Q.o;
  return L;
}

// ---- vieo_tracker_multi_create's steps

// the sizes of the blocks for max_seq frames and the offsets of the fixed ones' arrays
static void multi_layout_blocks(vieo_tracker_multi* m) {
  Layout Lo, W, C;  // local maps, work, constants
  const size_t M = m->max_seq, kc = m->kc, cap = m->cap, ccap = m->ccap, pcap = m->pcap;
  const MultiLayout L = multi_layout(m, m->max_seq);
  m->up_bytes = L.u_imu + M * m->imu_cap * sizeof(vieo_imu_sample), m->out_bytes = L.q_end, m->img_bytes = M * 2 * m->npx;
  m->l_pts = Lo.take(M * ccap * sizeof(vieo_frustum_point)), m->l_desc = Lo.take(M * ccap * 32), m->l_xyz = Lo.take(M * ccap * 12);
  m->loc_bytes = Lo.o;
  m->w_kp = W.take(2 * M * cap * sizeof(vieo_keypoint)), m->w_desc = W.take(2 * M * cap * 32);
  m->w_q1 = W.take(M * kc * sizeof(vieo_proj_query)), m->w_q2 = W.take(M * ccap * sizeof(vieo_proj_query));
  m->w_assign = W.take(M * kc * 4), m->w_taken = W.take(M * kc), m->w_held = W.take(M * pcap);
  m->w_obs = W.take(M * kc * sizeof(vieo_pose_obs)), m->w_obskey = W.take(M * kc * 4), m->w_outl = W.take(M * kc);
  m->w_xyz = W.take(M * pcap * 12), m->w_dep = W.take(M * pcap * 4);
  m->w_pre = W.take(M * sizeof(vieo_imu_preint)), m->w_prv = W.take(M * 81 * 8), m->w_pst = W.take(M * 4),
      m->w_bias = W.take(M * 6 * 8);
  m->work_bytes = W.o;
  (void)C.take(sizeof(vieo_imu_noise));
  m->c_consts = C.take(32 * 4);
  m->const_bytes = C.o;
}

// the pinned and device blocks, the second stream, the events; the blocks cleared
static bool multi_allocate(vieo_tracker_multi* m) {
  const auto pinned = [](uint8_t** p, size_t n) { return hipHostMalloc((void**)p, n, hipHostMallocDefault) == hipSuccess; };
  const auto device = [](uint8_t** p, size_t n) { return hipMalloc((void**)p, n) == hipSuccess; };
  bool ok = pinned(&m->h_up, m->up_bytes) && pinned(&m->h_img, m->img_bytes) && pinned(&m->h_loc, m->loc_bytes) &&
            pinned(&m->h_out, m->out_bytes) && device(&m->d_up, m->up_bytes) && device(&m->d_img, m->img_bytes) &&
            device(&m->d_loc, m->loc_bytes) && device(&m->d_out, m->out_bytes) && device(&m->d_work, m->work_bytes) &&
            device(&m->d_const, m->const_bytes) && create_side_stream(&m->st_imu, m->st, &m->side_ratio) == hipSuccess;
  for (hipEvent_t* e : {&m->ev_up, &m->ev_imu, &m->ev_ext, &m->ev_kd})
    ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipEventCreate(&m->ev_t0) == hipSuccess && hipEventCreate(&m->ev_t1) == hipSuccess;
  if (!ok) {
    set_error("vieo_tracker_multi_create: allocation failed (%s)", hipGetErrorString(hipGetLastError()));
    return false;
  }
  memset(m->h_up, 0, m->up_bytes), memset(m->h_out, 0, m->out_bytes);
  return true;
}

// the constant parts of a frame's records (vieo_tracker_create's header); what every frame shares goes up: the IMU
// noise, inv_sigma2 / scale of the levels
static bool multi_constants(vieo_tracker_multi* m) {
  float scale[16], inv_sigma2[16];
  vieo_orb_scale_factors(m->ext, scale);
  vieo_orb_inv_level_sigma2(m->ext, inv_sigma2);
  track_build_constants(m->K, m->P, scale, inv_sigma2, nullptr, nullptr);
  std::vector<uint8_t> cst(m->const_bytes, 0);
  memcpy(cst.data(), &m->P.noise, sizeof(vieo_imu_noise));
  memcpy(cst.data() + m->c_consts, m->K.consts, sizeof(m->K.consts));
  const bool ok = hipMemsetAsync(m->d_work, 0, m->work_bytes, m->st) == hipSuccess &&
                  hipMemsetAsync(m->d_out, 0, m->out_bytes, m->st) == hipSuccess &&
                  hipMemsetAsync(m->d_loc, 0, m->loc_bytes, m->st) == hipSuccess &&
                  hipMemcpyAsync(m->d_const, cst.data(), m->const_bytes, hipMemcpyHostToDevice, m->st) == hipSuccess &&
                  hipStreamSynchronize(m->st) == hipSuccess;
  if (!ok) set_error("vieo_tracker_multi_create: initialisation failed (%s)", hipGetErrorString(hipGetLastError()));
  return ok;
}

extern "C" {

void vieo_tracker_multi_destroy(vieo_tracker_multi* m) {
  if (!m) return;
  if (m->st) (void)hipStreamSynchronize(m->st);
  if (m->st_imu) (void)hipStreamSynchronize(m->st_imu), (void)hipStreamDestroy(m->st_imu);
  for (hipEvent_t e : {m->ev_up, m->ev_imu, m->ev_ext, m->ev_kd, m->ev_t0, m->ev_t1})
    if (e) (void)hipEventDestroy(e);
  for (uint8_t* p : {m->h_up, m->h_img, m->h_loc, m->h_out})
    if (p) (void)hipHostFree(p);
  for (uint8_t* p : {m->d_up, m->d_img, m->d_loc, m->d_out, m->d_work, m->d_const})
    if (p) (void)hipFree(p);
  if (m->ext) vieo_orb_destroy(m->ext);
  delete m;
}

int vieo_tracker_multi_create(vieo_tracker_multi** out, const vieo_tracker_params* P, int max_sequences) {
  // (vieo_tracker_create's checks, then the slot count: above 256 frames the pose optimisation's kernel instance changes)
  if (!out || !P || P->width <= 0 || P->height <= 0 || P->n_levels < 1 || P->n_levels > 16 || P->max_local_points < 0)
    return VIEO_E_INVALID;
  if (max_sequences < 1 || max_sequences > 256) {
    set_error("vieo_tracker_multi_create: max_sequences = %d (1..256)", max_sequences);
    return VIEO_E_INVALID;
  }
  int rc = require_device();
  if (rc != VIEO_OK) return rc;
  vieo_tracker_multi* m = new vieo_tracker_multi();
  m->P = *P, m->vision = P->vision_only != 0, m->max_seq = max_sequences;
  if ((rc = vieo::orb_create_with_priority(&m->ext, P->n_features, P->scale_factor, P->n_levels, P->ini_th_fast, P->min_th_fast,
                                           track_main_priority())) != VIEO_OK) {
    delete m;
    return rc;
  }
  m->st = (hipStream_t)vieo_orb_stream(m->ext);
  m->cap = m->kc = vieo_orb_max_keypoints(m->ext);
  m->ccap = std::max(P->max_local_points, 64), m->pcap = m->kc + m->ccap;
  m->fstride = m->vision ? sizeof(vieo_pose_frame) : sizeof(vieo_vio_frame);
  m->rstride = m->vision ? sizeof(vieo_pose_result) : sizeof(vieo_vio_result);
  m->local_version.assign(max_sequences, -1), m->n_local_dev.assign(max_sequences, 0);
  m->npx = (size_t)P->width * P->height;
  multi_layout_blocks(m);
  if (!multi_allocate(m) || !multi_constants(m)) {
    vieo_tracker_multi_destroy(m);
    return VIEO_E_HIP;
  }
  *out = m;
  return VIEO_OK;
}

int vieo_tracker_multi_image_buffer(vieo_tracker_multi* m, int slot, int image_index, uint8_t** plane) {
  if (!m || !plane || slot < 0 || slot >= m->max_seq || image_index < 0 || image_index > 1) return VIEO_E_INVALID;
  *plane = m->h_img + ((size_t)slot * 2 + image_index) * m->npx;
  return VIEO_OK;
}

int vieo_tracker_multi_reset_slot(vieo_tracker_multi* m, int slot) {
  if (!m || slot < 0 || slot >= m->max_seq) return VIEO_E_INVALID;
  m->local_version[slot] = -1, m->n_local_dev[slot] = 0;  // (a fresh vieo_tracker's state)
  return VIEO_OK;
}

}  // extern "C"

// ---- vieo_track_frames: a call record and the stages that work on it
struct MultiCall {
  vieo_tracker_multi* m;
  int n;
  const int32_t* slots;
  const vieo_track_input* in;
  vieo_track_output* out;
  MultiLayout L;
  std::vector<uint8_t> new_local, widened;  // per frame: its slot's local map changed / it took the wider window
  int total_imu = 0, max_local = 0;
  TrackChain chain;
  std::chrono::steady_clock::time_point t_enter;
};

// the call's arrays as the chain reads them (n frames)
static TrackChain multi_chain(const vieo_tracker_multi* m, const MultiLayout& L, int n) {
  uint8_t *U = m->d_up, *O = m->d_out, *W = m->d_work;
  TrackChain c;
  c.n = n, c.kc = m->kc, c.pcap = m->pcap, c.n_cams = 1, c.rig = false, c.vision = m->vision, c.st = m->st;
  c.kp = (const vieo_keypoint*)(W + m->w_kp), c.desc = W + m->w_desc, c.uright = (const float*)(O + L.q_ur);
  c.cnt = (const int32_t*)(O + L.q_cnt), c.cam_first = nullptr, c.bounds = m->K.bounds[0];
  c.q1 = (const vieo_proj_query*)(W + m->w_q1), c.nq1 = (const int32_t*)(U + L.u_nl), c.q1_cap = m->kc, c.same_point = nullptr,
      c.query_src = nullptr;
  c.q2 = (vieo_proj_query*)(W + m->w_q2), c.nq2 = (int32_t*)(O + L.q_nq2), c.q2_cap = m->ccap;
  c.assign = (int32_t*)(W + m->w_assign), c.taken = W + m->w_taken, c.held = W + m->w_held, c.mpref = (int32_t*)(O + L.q_mpref);
  c.obs = (vieo_pose_obs*)(W + m->w_obs), c.obskey = (int32_t*)(W + m->w_obskey), c.outl = W + m->w_outl, c.key_outlier = O + L.q_outl;
  c.xyz = (float*)(W + m->w_xyz), c.dep = (float*)(W + m->w_dep), c.consts = (const float*)(m->d_const + m->c_consts);
  c.f1 = U + L.u_f1, c.f2 = U + L.u_f2, c.r1 = O + L.q_r1, c.r2 = O + L.q_r2, c.fstride = m->fstride;
  c.nm1 = (int32_t*)(O + L.q_nm1), c.nm2 = (int32_t*)(O + L.q_nm2), c.nobs2 = (int32_t*)(O + L.q_nobs);
  c.nn_last = m->P.nn_last, c.nn_local = m->P.nn_local, c.close = std::max(10.0f, m->P.th_depth);
  return c;
}

// every frame is checked before anything is written or launched
static int multi_check(MultiCall& c) {
  vieo_tracker_multi* m = c.m;
  const int n = c.n;
  if (n < 1 || n > m->max_seq) {
    set_error("vieo_track_frames: %d frames (1..%d per call)", n, m->max_seq);
    return VIEO_E_INVALID;
  }
  std::vector<uint8_t> seen(m->max_seq, 0);
  c.new_local.assign(n, 0), c.widened.assign(n, 0);
  for (int i = 0; i < n; i++) {
    const int s = c.slots[i];
    if (s < 0 || s >= m->max_seq || seen[s]) {
      set_error("vieo_track_frames: frame %d: slot %d is out of range (0..%d) or appears twice", i, s, m->max_seq - 1);
      return VIEO_E_INVALID;
    }
    seen[s] = 1;
    const vieo_track_input* I = c.in + i;
    if (!track_input_ok(*I, m->P.width) || !I->left || !I->right) {
      set_error("vieo_track_frames: slot %d: invalid input (stride, counts, null arrays or images)", s);
      return VIEO_E_INVALID;
    }
    if (I->next_left || I->next_right || I->next_imu || I->use_prefetched || I->next_images[0] || I->next_images[1] ||
        I->next_images[2] || I->next_images[3]) {
      set_error("vieo_track_frames: slot %d: frame pipelining (next_* / use_prefetched) is not offered here", s);
      return VIEO_E_INVALID;
    }
    if (!track_input_fits(*I, m->kc, m->ccap, m->imu_cap)) {
      set_error("vieo_track_frames: slot %d: %d last-frame points / %d local points / %d IMU samples exceed the capacities "
                "%d / %d / %d", s, I->n_last, I->n_local, I->n_imu, m->kc, m->ccap, m->imu_cap);
      return VIEO_E_CAPACITY;
    }
    c.new_local[i] = track_local_changed(*I, m->local_version[s], m->n_local_dev[s]);
    if (c.new_local[i] && (!I->local_points || !I->local_desc)) {
      set_error("vieo_track_frames: slot %d: a changed local map needs local_points and local_desc", s);
      return VIEO_E_INVALID;
    }
    c.total_imu += m->vision ? 0 : I->n_imu, c.max_local = std::max(c.max_local, (int)I->n_local);
  }
  const int rc = require_device();
  if (rc != VIEO_OK) return rc;
  c.t_enter = std::chrono::steady_clock::now();
  c.L = multi_layout(m, n);
  c.chain = multi_chain(m, c.L, n);
  return VIEO_OK;
}

// the pinned blocks: the frames' records, IMU samples, last points, aliases; images and changed local maps into their slots
static void multi_fill_upload(MultiCall& c) {
  vieo_tracker_multi* m = c.m;
  const MultiLayout& L = c.L;
  const int kc = m->kc, ccap = m->ccap;
  uint8_t* H = m->h_up;
  vieo_sbp_camera* cam = (vieo_sbp_camera*)(H + L.u_cam);
  vieo_navstate *nref = (vieo_navstate*)(H + L.u_nref), *nlast = (vieo_navstate*)(H + L.u_nlast);
  double *ti = (double*)(H + L.u_ti), *tj = (double*)(H + L.u_tj), *bg = (double*)(H + L.u_bg), *ba = (double*)(H + L.u_ba);
  int32_t *first = (int32_t*)(H + L.u_first), *nl = (int32_t*)(H + L.u_nl), *nloc = (int32_t*)(H + L.u_nloc),
      *pslot = (int32_t*)(H + L.u_slot);
  vieo_imu_sample* samples = (vieo_imu_sample*)(H + L.u_imu);
  first[0] = 0;
  for (int i = 0; i < c.n; i++) {
    const vieo_track_input* I = c.in + i;
    const int s = c.slots[i];
    cam[i] = m->K.cam0;
    for (int which = 0; which < 2; which++) {
      vieo_vio_frame f = which ? m->K.f2_0 : m->K.f1_0;
      track_fill_problem(f, *I);
      memcpy(H + (which ? L.u_f2 : L.u_f1) + (size_t)i * m->fstride, &f, m->fstride);  // (vision-only: the leading vieo_pose_frame)
    }
    nref[i] = I->nav_ref, nlast[i] = I->nav_last, ti[i] = I->t_ref, tj[i] = I->t_cur;
    for (int k = 0; k < 3; k++) bg[3 * i + k] = I->nav_ref.bg[k], ba[3 * i + k] = I->nav_ref.ba[k];
    const int ni = m->vision ? 0 : I->n_imu;
    if (ni) memcpy(samples + first[i], I->imu, (size_t)ni * sizeof(vieo_imu_sample));
    first[i + 1] = first[i] + ni;
    nl[i] = I->n_last, nloc[i] = I->n_local, pslot[i] = s;
    if (I->n_last) {
      memcpy(H + L.u_pts + (size_t)i * kc * sizeof(vieo_last_frame_point), I->last_points,
             (size_t)I->n_last * sizeof(vieo_last_frame_point));
      track_pack_xyz((float*)(H + L.u_xyz) + (size_t)i * kc * 3, I->last_points, I->n_last);
      memcpy((float*)(H + L.u_dep) + (size_t)i * kc, I->last_track_depth, (size_t)I->n_last * 4);
    }
    if (I->n_local) memcpy((int32_t*)(H + L.u_alias) + (size_t)i * ccap, I->local_alias, (size_t)I->n_local * 4);
    for (int e = 0; e < 2; e++)
      track_copy_plane(m->h_img + ((size_t)s * 2 + e) * m->npx, e ? I->right : I->left, m->P.width, m->P.height, I->stride);
    if (c.new_local[i]) {
      const int nc = I->n_local;
      memcpy(m->h_loc + m->l_pts + (size_t)s * ccap * sizeof(vieo_frustum_point), I->local_points,
             (size_t)nc * sizeof(vieo_frustum_point));
      memcpy(m->h_loc + m->l_desc + (size_t)s * ccap * 32, I->local_desc, (size_t)nc * 32);
      track_pack_xyz((float*)(m->h_loc + m->l_xyz) + (size_t)s * ccap * 3, I->local_points, nc);
    }
  }
}

// the first search's queries from the predicted poses
static int multi_project(const MultiCall& c, hipStream_t s) {
  const vieo_tracker_multi* m = c.m;
  return vieo_sbp_project_last_frame_batch_device((const vieo_last_frame_point*)(m->d_up + c.L.u_pts),
                                                  (const int32_t*)(m->d_up + c.L.u_nl),
                                                  m->kc, c.n, (const vieo_sbp_camera*)(m->d_up + c.L.u_cam),
                                                  (vieo_proj_query*)(m->d_work + m->w_q1), s);
}

// One copy up (+ the images) and the extraction of the 2n images; beside it the second stream's work; the stereo stage.
static int multi_head(MultiCall& c) {
  vieo_tracker_multi* m = c.m;
  const MultiLayout& L = c.L;
  const int n = c.n;
  const size_t npx = m->npx;
  hipStream_t st = m->st;
  uint8_t *U = m->d_up, *O = m->d_out, *Wk = m->d_work;
  VIEO_HIP_CHECK(hipEventRecord(m->ev_t0, st));
  VIEO_HIP_CHECK(hipMemcpyAsync(m->d_up, m->h_up, L.u_imu + (size_t)c.total_imu * sizeof(vieo_imu_sample), hipMemcpyHostToDevice, st));
  VIEO_HIP_CHECK(hipEventRecord(m->ev_up, st));
  // (the unwritten last word of a vieo_vio_result stays zero, as in vieo_tracker's download block)
  VIEO_HIP_CHECK(hipMemsetAsync(O + L.q_r1, 0, 2 * (size_t)n * m->rstride, st));
  for (int i = 0; i < n;) {  // the planes of runs of consecutive slots in one copy each
    int j = i + 1;
    while (j < n && c.slots[j] == c.slots[j - 1] + 1) j++;
    VIEO_HIP_CHECK(hipMemcpyAsync(m->d_img + (size_t)i * 2 * npx, m->h_img + (size_t)c.slots[i] * 2 * npx, (size_t)(j - i) * 2 * npx,
                                  hipMemcpyHostToDevice, st));
    i = j;
  }
  int rc = vieo_orb_extract_batch_device(m->ext, m->d_img, 2 * n, m->P.width, m->P.height, m->P.width, npx, nullptr,
                                         (vieo_keypoint*)(Wk + m->w_kp),
                                         Wk + m->w_desc, m->cap, (int32_t*)(O + L.q_cnt));
  if (rc != VIEO_OK) return rc;
  // The second stream (handed over behind the extraction's launches, the head of the critical path): the changed local
  // maps, the pre-integrations, the predictions and point tables, the first search's queries
  const int kc = m->kc, ccap = m->ccap;
  hipStream_t sb = m->st_imu;
  VIEO_HIP_CHECK(hipStreamWaitEvent(sb, m->ev_up, 0));
  for (int i = 0; i < n; i++) {
    if (!c.new_local[i]) continue;
    const int s = c.slots[i], nc = c.in[i].n_local;
    const size_t op = m->l_pts + (size_t)s * ccap * sizeof(vieo_frustum_point), od = m->l_desc + (size_t)s * ccap * 32,
        ox = m->l_xyz + (size_t)s * ccap * 12;
    VIEO_HIP_CHECK(hipMemcpyAsync(m->d_loc + op, m->h_loc + op, (size_t)nc * sizeof(vieo_frustum_point), hipMemcpyHostToDevice, sb));
    VIEO_HIP_CHECK(hipMemcpyAsync(m->d_loc + od, m->h_loc + od, (size_t)nc * 32, hipMemcpyHostToDevice, sb));
    VIEO_HIP_CHECK(hipMemcpyAsync(m->d_loc + ox, m->h_loc + ox, (size_t)nc * 12, hipMemcpyHostToDevice, sb));
  }
  const MultiTables tables{(const float*)(U + L.u_xyz), (const float*)(U + L.u_dep), (const float*)(m->d_loc + m->l_xyz),
                           (float*)(Wk + m->w_xyz),
                           (float*)(Wk + m->w_dep), (const int32_t*)(U + L.u_nl), (const int32_t*)(U + L.u_nloc),
                           (const int32_t*)(U + L.u_slot), kc, ccap, m->pcap};
  if (!m->vision) {
    if ((rc = vieo_imu_preintegrate_batch_device((const vieo_imu_noise*)m->d_const, (const vieo_imu_sample*)(U + L.u_imu),
                                                 (const int32_t*)(U + L.u_first), (const double*)(U + L.u_ti),
                                                 (const double*)(U + L.u_tj),
                                                 (const double*)(U + L.u_bg), (const double*)(U + L.u_ba), n,
                                                 (vieo_imu_preint*)(Wk + m->w_pre),
                                                 (double*)(Wk + m->w_prv), (int32_t*)(Wk + m->w_pst), sb)) != VIEO_OK)
      return rc;
    hipLaunchKernelGGL(k_track_predict_multi, dim3(1 + kTableBlocks, n), dim3(64), 0, sb, (const vieo_navstate*)(U + L.u_nref),
                       (const vieo_navstate*)(U + L.u_nlast), (vieo_vio_frame*)(U + L.u_f1), (vieo_vio_frame*)(U + L.u_f2),
                       (vieo_sbp_camera*)(U + L.u_cam),
                       (vieo_navstate*)(O + L.q_nav), (vieo_imu_preint*)(O + L.q_imu), (double*)(O + L.q_sig), (int32_t*)(O + L.q_pst),
                       (const vieo_imu_preint*)(Wk + m->w_pre), (const double*)(Wk + m->w_prv), (const int32_t*)(Wk + m->w_pst),
                       (double*)(Wk + m->w_bias), tables);
  } else {
    hipLaunchKernelGGL(k_track_set_pose_multi, dim3(1 + kTableBlocks, n), dim3(64), 0, sb, (const vieo_navstate*)(U + L.u_nref),
                       (const vieo_navstate*)(U + L.u_nlast), (vieo_pose_frame*)(U + L.u_f1), (vieo_pose_frame*)(U + L.u_f2),
                       (vieo_sbp_camera*)(U + L.u_cam), (vieo_navstate*)(O + L.q_nav), (int32_t*)(O + L.q_pst), tables);
  }
  VIEO_HIP_CHECK(hipGetLastError());
  if ((rc = multi_project(c, sb)) != VIEO_OK) return rc;
  VIEO_HIP_CHECK(hipEventRecord(m->ev_imu, sb));
  // ComputeStereoMatches of the n frames; the left images' keys / descriptors back on the second stream, beside the chain
  const size_t cap = m->cap;
  vieo_keypoint* d_kp = (vieo_keypoint*)(Wk + m->w_kp);
  uint8_t* d_desc = Wk + m->w_desc;
  if ((rc = vieo_stereo_match_rectified_batch_device(m->ext, n, d_kp, d_desc, (int32_t*)(O + L.q_cnt), m->cap, m->P.baseline, m->P.bf,
                                                     (float*)(O + L.q_ur), (float*)(O + L.q_dp))) != VIEO_OK)
    return rc;
  VIEO_HIP_CHECK(hipEventRecord(m->ev_ext, m->st));
  VIEO_HIP_CHECK(hipStreamWaitEvent(sb, m->ev_ext, 0));
  VIEO_HIP_CHECK(hipMemcpy2DAsync(m->h_out + L.q_kp, cap * sizeof(vieo_keypoint), d_kp, 2 * cap * sizeof(vieo_keypoint),
                                  cap * sizeof(vieo_keypoint), n, hipMemcpyDeviceToHost, sb));
  VIEO_HIP_CHECK(hipMemcpy2DAsync(m->h_out + L.q_desc, cap * 32, d_desc, 2 * cap * 32, cap * 32, n, hipMemcpyDeviceToHost, sb));
  VIEO_HIP_CHECK(hipEventRecord(m->ev_kd, sb));
  return VIEO_OK;
}

// The chain behind the prediction over all n frames, the copies back and the host's wait.  first: the call's first run --
// the first search's queries are there (second stream: joined here), as are the keys' / descriptors' copies; a repeat projects again.
static int multi_tail(MultiCall& c, bool first) {
  vieo_tracker_multi* m = c.m;
  const MultiLayout& L = c.L;
  const TrackChain& ch = c.chain;
  hipStream_t st = m->st;
  if (first) VIEO_HIP_CHECK(hipStreamWaitEvent(st, m->ev_imu, 0));
  const int rc = track_run_chain(
      ch, first, [&] { return multi_project(c, st); }, [] { return (int)VIEO_OK; },
      [&] {
        return vieo_track_local_queries_slot_batch_device(&m->K.ff, ch.f1, ch.fstride, ch.r1, m->rstride, ch.n,
                                                          (const int32_t*)(m->d_up + L.u_slot),
                                                          (const vieo_frustum_point*)(m->d_loc + m->l_pts), m->d_loc + m->l_desc,
                                                          (const int32_t*)(m->d_up + L.u_alias), (const int32_t*)(m->d_up + L.u_nloc),
                                                          m->ccap, ch.held, ch.pcap, m->P.th_local, 0.f, ch.consts + 16, ch.q2,
                                                          ch.dep + ch.kc, ch.pcap, ch.nq2, st);
      });
  if (rc != VIEO_OK) return rc;
  // results: [headers | uright | depth | point_ref | outlier] of the n frames, and the candidates' depths
  VIEO_HIP_CHECK(hipMemcpyAsync(m->h_out, m->d_out, L.q_small, hipMemcpyDeviceToHost, st));
  if (c.max_local > 0)
    VIEO_HIP_CHECK(hipMemcpy2DAsync(m->h_out + L.q_cdep, (size_t)m->ccap * 4, ch.dep + ch.kc, (size_t)ch.pcap * 4,
                                    (size_t)c.max_local * 4,
                                    ch.n, hipMemcpyDeviceToHost, st));
  if (first) VIEO_HIP_CHECK(hipStreamWaitEvent(st, m->ev_kd, 0));
  VIEO_HIP_CHECK(hipEventRecord(m->ev_t1, st));
  VIEO_HIP_CHECK(hipStreamSynchronize(st));
  return VIEO_OK;
}

// Tracking.cc:301-309 / :1869-1876: the wider window for the frames that want it; the chain runs again over all frames
static int multi_wider_window(MultiCall& c) {
  vieo_tracker_multi* m = c.m;
  const MultiLayout& L = c.L;
  const int32_t *nm1 = (const int32_t*)(m->h_out + L.q_nm1), *pst = (const int32_t*)(m->h_out + L.q_pst);
  const vieo_imu_preint* imu = (const vieo_imu_preint*)(m->h_out + L.q_imu);
  vieo_sbp_camera* cam = (vieo_sbp_camera*)(m->h_up + L.u_cam);
  int n_wide = 0;
  for (int i = 0; i < c.n; i++) {
    if (!track_wants_wider_window(track_pre_ok(m->vision, pst[i], imu[i].dt), nm1[i])) continue;
    c.widened[i] = 1, n_wide++;
    cam[i].th = 2 * m->P.th_last;
    const size_t at = L.u_cam + (size_t)i * sizeof(vieo_sbp_camera) + offsetof(vieo_sbp_camera, th);
    VIEO_HIP_CHECK(hipMemcpyAsync(m->d_up + at, &cam[i].th, 4, hipMemcpyHostToDevice, m->st));
  }
  return n_wide ? multi_tail(c, false) : VIEO_OK;
}

static void multi_output(MultiCall& c) {
  vieo_tracker_multi* m = c.m;
  const MultiLayout& L = c.L;
  const size_t cap = m->cap, kc = m->kc;
  for (int i = 0; i < c.n; i++)
    if (c.new_local[i]) m->local_version[c.slots[i]] = c.in[i].local_version, m->n_local_dev[c.slots[i]] = c.in[i].n_local;
  float ms_gpu = 0;
  (void)hipEventElapsedTime(&ms_gpu, m->ev_t0, m->ev_t1);
  const float ms_host = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - c.t_enter).count();
  const uint8_t* Q = m->h_out;
  const int32_t *cnt = (const int32_t*)(Q + L.q_cnt), *nm1 = (const int32_t*)(Q + L.q_nm1), *nm2 = (const int32_t*)(Q + L.q_nm2),
      *pst = (const int32_t*)(Q + L.q_pst);
  const vieo_imu_preint* imu = (const vieo_imu_preint*)(Q + L.q_imu);
  for (size_t i = 0; i < (size_t)c.n; i++) {
    vieo_track_output* o = c.out + i;
    track_fill_output(o, m->vision, pst[i], nm1[i], nm2[i], c.widened[i], ((const vieo_navstate*)(Q + L.q_nav))[i],
                      m->vision ? nullptr : imu + i,
                      Q + L.q_r1 + i * m->rstride, Q + L.q_r2 + i * m->rstride, m->rstride, ms_gpu, ms_host);
    o->n_keys = o->cam_first[1] = std::min(cnt[4 * i], m->cap), o->key_cap = m->kc;
    o->keys = (const vieo_keypoint*)(Q + L.q_kp) + i * cap, o->desc = Q + L.q_desc + i * cap * 32;
    o->uright = (const float*)(Q + L.q_ur) + i * kc, o->depth = (const float*)(Q + L.q_dp) + i * kc;
    o->point_ref = (const int32_t*)(Q + L.q_mpref) + i * kc, o->outlier = Q + L.q_outl + i * kc;
    o->local_track_depth = (const float*)(Q + L.q_cdep) + i * m->ccap;
  }
}

// an error in the middle: work queued on the two streams still reads the pinned blocks -- wait for it
static int multi_fail(vieo_tracker_multi* m, int rc) {
  (void)hipStreamSynchronize(m->st_imu);
  (void)hipStreamSynchronize(m->st);
  return rc;
}

extern "C" {

int vieo_track_frames(vieo_tracker_multi* m, int n, const int32_t* slots, const vieo_track_input* in, vieo_track_output* out) {
  if (!m || !slots || !in || !out) return VIEO_E_INVALID;
  MultiCall c{m, n, slots, in, out};
  int rc = multi_check(c);
  if (rc != VIEO_OK) return rc;
  multi_fill_upload(c);
  // the launches, in stream order; a failure waits for what is queued (multi_fail)
  if ((rc = multi_head(c)) != VIEO_OK || (rc = multi_tail(c, true)) != VIEO_OK || (rc = multi_wider_window(c)) != VIEO_OK)
    return multi_fail(m, rc);
  multi_output(c);
  return VIEO_OK;
}

}  // extern "C"
