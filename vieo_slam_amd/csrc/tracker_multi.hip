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
//              -> PoseOptimization(bComputeMarg) [n] -> k_track_finish_multi
//   D2H, ONE host synchronisation (+ the tail again over all n frames when one of them takes the wider window).
//
// Every stage computes a frame from that frame's data alone, in fixed orders (no floating-point atomics): a frame's bytes
// do not depend on the batch it is in, and equal what vieo_track_frame gives for it.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "orb_internal.h"
#include "track_predict.h"

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

// per-key outlier flags of the second optimisation (mvbOutlier) and its observation count, one workgroup per frame;
// f2: vieo_vio_frame or vieo_pose_frame records, f2_stride bytes apart (both start with the vieo_pose_frame)
__global__ void __launch_bounds__(256)
k_track_finish_multi(const int32_t* __restrict__ obs_key, const uint8_t* __restrict__ outl, const uint8_t* __restrict__ f2,
                     size_t f2_stride, uint8_t* __restrict__ key_outlier, int key_cap, int32_t* __restrict__ nobs2) {
  const size_t i = blockIdx.x;
  const int n = ((const vieo_pose_frame*)(f2 + i * f2_stride))->n_obs;
  obs_key += i * key_cap, outl += i * key_cap, key_outlier += i * key_cap;
  for (int k = threadIdx.x; k < key_cap; k += 256) key_outlier[k] = 0;
  __syncthreads();
  for (int j = threadIdx.x; j < n; j += 256)
    if (outl[j]) key_outlier[obs_key[j]] = 1;
  if (threadIdx.x == 0) nobs2[i] = n;
}

static size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

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
  float scale[16], inv_sigma2[16];
  vieo_camera pin_cam;
  vieo_frustum_frame ff;
  float bounds[4];
  vieo_sbp_camera cam0;       // the constant part of a frame's search camera
  vieo_vio_frame f1_0, f2_0;  // ... and of its two optimiser problems
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
  size_t c_consts;
  size_t w_kp, w_desc, w_q1, w_q2, w_assign, w_taken, w_held, w_obs, w_obskey, w_outl, w_xyz, w_dep, w_pre, w_prv, w_pst, w_bias;
};

static MultiLayout multi_layout(const vieo_tracker_multi* m, int n) {
  MultiLayout L;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t r = o;
    o = al256(o + bytes);
    return r;
  };
  const size_t N = n;
  L.u_cam = take(N * sizeof(vieo_sbp_camera)), L.u_f1 = take(N * m->fstride), L.u_f2 = take(N * m->fstride);
  L.u_nref = take(N * sizeof(vieo_navstate)), L.u_nlast = take(N * sizeof(vieo_navstate));
  L.u_ti = take(N * 8), L.u_tj = take(N * 8), L.u_bg = take(N * 24), L.u_ba = take(N * 24), L.u_first = take((N + 1) * 4);
  L.u_nl = take(N * 4), L.u_nloc = take(N * 4), L.u_slot = take(N * 4);
  L.u_pts = take(N * m->kc * sizeof(vieo_last_frame_point)), L.u_xyz = take(N * m->kc * 12), L.u_dep = take(N * m->kc * 4);
  L.u_alias = take(N * m->ccap * 4);
  L.u_imu = take(N * m->imu_cap * sizeof(vieo_imu_sample));  // (last: a call uploads up to its samples)
  o = 0;
  L.q_cnt = take(N * 2 * 8), L.q_nm1 = take(N * 4), L.q_nm2 = take(N * 4), L.q_nq2 = take(N * 4), L.q_pst = take(N * 4);
  L.q_nobs = take(N * 4), L.q_r1 = o, o += N * m->rstride, L.q_r2 = o, o = al256(o + N * m->rstride);  // (adjacent: one clear)
  L.q_nav = take(N * sizeof(vieo_navstate)), L.q_imu = take(N * sizeof(vieo_imu_preint)), L.q_sig = take(N * 81 * 8);
  L.q_ur = take(N * m->kc * 4), L.q_dp = take(N * m->kc * 4), L.q_mpref = take(N * m->kc * 4), L.q_outl = take(N * m->kc);
  L.q_small = o;
  L.q_kp = take(N * m->cap * sizeof(vieo_keypoint)), L.q_desc = take(N * m->cap * 32), L.q_cdep = take(N * m->ccap * 4);
  L.q_end = o;
  return L;
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
  m->P = *P;
  m->vision = P->vision_only != 0;
  m->max_seq = max_sequences;
  static const int main_prio = [] {  // (as vieo_tracker: VIEO_TRACKER_PRIORITY=0 puts every stream at normal priority)
    const char* e = getenv("VIEO_TRACKER_PRIORITY");
    return e ? atoi(e) : 1;
  }();
  if ((rc = vieo::orb_create_with_priority(&m->ext, P->n_features, P->scale_factor, P->n_levels, P->ini_th_fast, P->min_th_fast,
                                           main_prio)) != VIEO_OK) {
    delete m;
    return rc;
  }
  m->st = (hipStream_t)vieo_orb_stream(m->ext);
  m->cap = vieo_orb_max_keypoints(m->ext);
  m->kc = m->cap;
  m->ccap = std::max(P->max_local_points, 64);
  m->pcap = m->kc + m->ccap;
  m->fstride = m->vision ? sizeof(vieo_pose_frame) : sizeof(vieo_vio_frame);
  m->rstride = m->vision ? sizeof(vieo_pose_result) : sizeof(vieo_vio_result);
  m->local_version.assign(max_sequences, -1), m->n_local_dev.assign(max_sequences, 0);
  vieo_orb_scale_factors(m->ext, m->scale);
  vieo_orb_inv_level_sigma2(m->ext, m->inv_sigma2);
  m->npx = (size_t)P->width * P->height;
  const size_t M = max_sequences, kc = m->kc, cap = m->cap, ccap = m->ccap, pcap = m->pcap;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t r = o;
    o = al256(o + bytes);
    return r;
  };
  const MultiLayout L = multi_layout(m, max_sequences);
  const size_t up_bytes = L.u_imu + M * m->imu_cap * sizeof(vieo_imu_sample), out_bytes = L.q_end;
  m->l_pts = take(M * ccap * sizeof(vieo_frustum_point)), m->l_desc = take(M * ccap * 32), m->l_xyz = take(M * ccap * 12);
  const size_t loc_bytes = o;
  o = 0;
  m->w_kp = take(2 * M * cap * sizeof(vieo_keypoint)), m->w_desc = take(2 * M * cap * 32);
  m->w_q1 = take(M * kc * sizeof(vieo_proj_query)), m->w_q2 = take(M * ccap * sizeof(vieo_proj_query));
  m->w_assign = take(M * kc * 4), m->w_taken = take(M * kc), m->w_held = take(M * pcap);
  m->w_obs = take(M * kc * sizeof(vieo_pose_obs)), m->w_obskey = take(M * kc * 4), m->w_outl = take(M * kc);
  m->w_xyz = take(M * pcap * 12), m->w_dep = take(M * pcap * 4);
  m->w_pre = take(M * sizeof(vieo_imu_preint)), m->w_prv = take(M * 81 * 8), m->w_pst = take(M * 4), m->w_bias = take(M * 6 * 8);
  const size_t work_bytes = o;
  o = 0;
  (void)take(sizeof(vieo_imu_noise));
  m->c_consts = take(32 * 4);
  const size_t const_bytes = o;
  const size_t img_bytes = M * 2 * m->npx;
  bool ok = hipHostMalloc((void**)&m->h_up, up_bytes, hipHostMallocDefault) == hipSuccess &&
            hipHostMalloc((void**)&m->h_img, img_bytes, hipHostMallocDefault) == hipSuccess &&
            hipHostMalloc((void**)&m->h_loc, loc_bytes, hipHostMallocDefault) == hipSuccess &&
            hipHostMalloc((void**)&m->h_out, out_bytes, hipHostMallocDefault) == hipSuccess &&
            hipMalloc((void**)&m->d_up, up_bytes) == hipSuccess && hipMalloc((void**)&m->d_img, img_bytes) == hipSuccess &&
            hipMalloc((void**)&m->d_loc, loc_bytes) == hipSuccess && hipMalloc((void**)&m->d_out, out_bytes) == hipSuccess &&
            hipMalloc((void**)&m->d_work, work_bytes) == hipSuccess && hipMalloc((void**)&m->d_const, const_bytes) == hipSuccess &&
            create_side_stream(&m->st_imu, m->st, &m->side_ratio) == hipSuccess &&
            hipEventCreateWithFlags(&m->ev_up, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&m->ev_imu, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&m->ev_ext, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&m->ev_kd, hipEventDisableTiming) == hipSuccess &&
            hipEventCreate(&m->ev_t0) == hipSuccess && hipEventCreate(&m->ev_t1) == hipSuccess;
  if (!ok) {
    set_error("vieo_tracker_multi_create: allocation failed (%s)", hipGetErrorString(hipGetLastError()));
    vieo_tracker_multi_destroy(m);
    return VIEO_E_HIP;
  }
  memset(m->h_up, 0, up_bytes), memset(m->h_out, 0, out_bytes);
  ok = hipMemsetAsync(m->d_work, 0, work_bytes, m->st) == hipSuccess && hipMemsetAsync(m->d_out, 0, out_bytes, m->st) == hipSuccess &&
       hipMemsetAsync(m->d_loc, 0, loc_bytes, m->st) == hipSuccess;
  // the constants every frame shares: the IMU noise, inv_sigma2 / scale of the levels
  std::vector<uint8_t> cst(const_bytes, 0);
  memcpy(cst.data(), &P->noise, sizeof(vieo_imu_noise));
  float* consts = (float*)(cst.data() + m->c_consts);
  for (int l = 0; l < P->n_levels; l++) consts[l] = m->inv_sigma2[l], consts[16 + l] = m->scale[l];
  ok = ok && hipMemcpyAsync(m->d_const, cst.data(), const_bytes, hipMemcpyHostToDevice, m->st) == hipSuccess &&
       hipStreamSynchronize(m->st) == hipSuccess;
  if (!ok) {
    set_error("vieo_tracker_multi_create: initialisation failed (%s)", hipGetErrorString(hipGetLastError()));
    vieo_tracker_multi_destroy(m);
    return VIEO_E_HIP;
  }
  // the constant parts of a frame's records (vieo_tracker_create's header)
  vieo_sbp_camera& C = m->cam0;
  memset(&C, 0, sizeof(C));
  C.fx = P->fx, C.fy = P->fy, C.cx = P->cx, C.cy = P->cy;
  C.bounds[0] = 0, C.bounds[1] = (float)P->width, C.bounds[2] = 0, C.bounds[3] = (float)P->height;
  C.bf = P->bf, C.baseline = P->baseline, C.th = P->th_last, C.th_far = 0;
  C.mono = 0, C.nlevels = P->n_levels;
  for (int l = 0; l < P->n_levels; l++) C.scale[l] = m->scale[l];
  m->bounds[0] = 0, m->bounds[1] = (float)P->width, m->bounds[2] = 0, m->bounds[3] = (float)P->height;
  memset(&m->f1_0, 0, sizeof(m->f1_0)), memset(&m->f2_0, 0, sizeof(m->f2_0));
  for (vieo_vio_frame* f : {&m->f1_0, &m->f2_0}) {
    memcpy(f->base.Rcb, P->Rcb, 72), memcpy(f->base.tcb, P->tcb, 24);
    f->base.fx = P->fx, f->base.fy = P->fy, f->base.cx = P->cx, f->base.cy = P->cy, f->base.bf = P->bf;
    memcpy(f->gw, P->gw, 24);
    f->inv_sigma_bg2 = P->inv_sigma_bg2, f->inv_sigma_ba2 = P->inv_sigma_ba2, f->th_depth = P->th_depth;
  }
  m->f2_0.compute_marg = 1;
  memset(&m->pin_cam, 0, sizeof(m->pin_cam));
  m->pin_cam.fx = P->fx, m->pin_cam.fy = P->fy, m->pin_cam.cx = P->cx, m->pin_cam.cy = P->cy;
  memset(&m->ff, 0, sizeof(m->ff));
  m->ff.n_cams = 1, m->ff.use_distort = 0, m->ff.cams = &m->pin_cam;
  m->ff.Tcr[0][0] = m->ff.Tcr[0][5] = m->ff.Tcr[0][10] = 1.f;
  for (int c = 0; c < 4; c++) memcpy(m->ff.bounds[c], m->bounds, 16);
  m->ff.bf = P->bf, m->ff.n_levels = P->n_levels, m->ff.viewing_cos_limit = 0.5f;
  m->ff.log_scale_factor = logf(P->scale_factor);
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

// the part of the chain behind the prediction, over all n frames: both searches and both optimisations, the copies back
static int multi_tail(vieo_tracker_multi* m, const MultiLayout& L, int n, int max_local, bool projected) {
  const vieo_tracker_params& P = m->P;
  const int kc = m->kc, ccap = m->ccap, pcap = m->pcap;
  hipStream_t st = m->st;
  uint8_t *U = m->d_up, *O = m->d_out, *W = m->d_work;
  const vieo_keypoint* d_kp = (const vieo_keypoint*)(W + m->w_kp);
  const uint8_t* d_desc = W + m->w_desc;
  const float* d_ur = (const float*)(O + L.q_ur);
  const int32_t* d_cnt = (const int32_t*)(O + L.q_cnt);
  const int32_t* d_nl = (const int32_t*)(U + L.u_nl);
  vieo_proj_query* d_q1 = (vieo_proj_query*)(W + m->w_q1);
  vieo_proj_query* d_q2 = (vieo_proj_query*)(W + m->w_q2);
  int32_t* d_assign = (int32_t*)(W + m->w_assign);
  int32_t* d_mpref = (int32_t*)(O + L.q_mpref);
  uint8_t* d_taken = W + m->w_taken;
  uint8_t* d_held = W + m->w_held;
  vieo_pose_obs* d_obs = (vieo_pose_obs*)(W + m->w_obs);
  int32_t* d_obskey = (int32_t*)(W + m->w_obskey);
  uint8_t* d_outl = W + m->w_outl;
  float* d_xyz = (float*)(W + m->w_xyz);
  float* d_dep = (float*)(W + m->w_dep);
  const float* consts = (const float*)(m->d_const + m->c_consts);
  const float close = std::max(10.0f, P.th_depth);
  const int vio = m->vision ? 0 : 1;
  uint8_t *f1 = U + L.u_f1, *f2 = U + L.u_f2, *r1 = O + L.q_r1, *r2 = O + L.q_r2;
  int rc;
#define MTRK(call)                           \
  do {                                       \
    if ((rc = (call)) != VIEO_OK) return rc; \
  } while (0)
  auto search = [&](int mode, const vieo_proj_query* q, const int32_t* d_nq, int q_cap, const uint8_t* taken, float nn, int32_t* d_nm) {
    return vieo_search_by_projection_batch_device(mode, q, d_nq, q_cap, n, d_kp, d_ur, d_desc, taken, d_cnt, kc, 0, 2, m->bounds,
                                                  nn, 1, d_assign, d_nm, st);
  };
  auto merge_build_obs = [&](void* frames, int point_offset, int reset) {
    return vieo_track_merge_build_obs_batch_device(d_assign, d_mpref, point_offset, reset, 1, nullptr, nullptr, 0, d_xyz,
                                                   m->vision ? nullptr : d_dep, close, pcap, d_kp, d_ur, d_cnt, nullptr, 1, kc, n,
                                                   0, 2, consts, d_obs, d_obskey, frames, vio, st);
  };
  auto pose = [&](void* frames, void* results) {
    if (m->vision)
      return vieo_pose_optimization_batch_device_ex((const vieo_pose_frame*)frames, n, d_obs, d_outl, (vieo_pose_result*)results,
                                                    VIEO_POSE_CAMS_RECTIFIED, st);
    return vieo_pose_optimization_vio_batch_device_ex((const vieo_vio_frame*)frames, n, d_obs, d_outl, (vieo_vio_result*)results,
                                                      VIEO_POSE_CAMS_RECTIFIED, VIEO_POSE_ENC_NONE, st);
  };
  if (!projected)
    MTRK(vieo_sbp_project_last_frame_batch_device((const vieo_last_frame_point*)(U + L.u_pts), d_nl, kc, n,
                                                  (const vieo_sbp_camera*)(U + L.u_cam), d_q1, st));
  MTRK(search(VIEO_SBP_LAST_FRAME, d_q1, d_nl, kc, nullptr, P.nn_last, (int32_t*)(O + L.q_nm1)));
  MTRK(merge_build_obs(f1, 0, 1));
  MTRK(pose(f1, r1));
  MTRK(vieo_track_after_pose_held_batch_device(d_mpref, d_obskey, d_outl, f1, r1, vio, kc, n, f2, d_taken, d_cnt, 0, 2, d_held,
                                               pcap, st));
  MTRK(vieo_track_local_queries_slot_batch_device(&m->ff, f1, m->fstride, r1, m->rstride, n, (const int32_t*)(U + L.u_slot),
                                                  (const vieo_frustum_point*)(m->d_loc + m->l_pts), m->d_loc + m->l_desc,
                                                  (const int32_t*)(U + L.u_alias), (const int32_t*)(U + L.u_nloc), ccap, d_held,
                                                  pcap, P.th_local, 0.f, consts + 16, d_q2, d_dep + kc, pcap,
                                                  (int32_t*)(O + L.q_nq2), st));
  (void)vieo_sbp_keep_grid(1);  // the frames' keys have not changed since the first search
  MTRK(search(VIEO_SBP_LOCAL_MAP, d_q2, (const int32_t*)(O + L.q_nq2), ccap, d_taken, P.nn_local, (int32_t*)(O + L.q_nm2)));
  MTRK(merge_build_obs(f2, kc, 0));
  MTRK(pose(f2, r2));
#undef MTRK
  hipLaunchKernelGGL(k_track_finish_multi, dim3(n), dim3(256), 0, st, d_obskey, d_outl, f2, m->fstride, O + L.q_outl, kc,
                     (int32_t*)(O + L.q_nobs));
  VIEO_HIP_CHECK(hipGetLastError());
  // results: [headers | uright | depth | point_ref | outlier] of the n frames, and the candidates' depths
  VIEO_HIP_CHECK(hipMemcpyAsync(m->h_out, O, L.q_small, hipMemcpyDeviceToHost, st));
  if (max_local > 0)
    VIEO_HIP_CHECK(hipMemcpy2DAsync(m->h_out + L.q_cdep, (size_t)ccap * 4, d_dep + kc, (size_t)pcap * 4, (size_t)max_local * 4, n,
                                    hipMemcpyDeviceToHost, st));
  return VIEO_OK;
}

extern "C" {

// an error in the middle of the chain: work queued on the two streams still reads the pinned blocks -- wait for it
static int multi_fail(vieo_tracker_multi* m, int rc) {
  (void)hipStreamSynchronize(m->st_imu);
  (void)hipStreamSynchronize(m->st);
  return rc;
}

int vieo_track_frames(vieo_tracker_multi* m, int n, const int32_t* slots, const vieo_track_input* in, vieo_track_output* out) {
  if (!m || !slots || !in || !out) return VIEO_E_INVALID;
  if (n < 1 || n > m->max_seq) {
    set_error("vieo_track_frames: %d frames (1..%d per call)", n, m->max_seq);
    return VIEO_E_INVALID;
  }
  const vieo_tracker_params& P = m->P;
  const int kc = m->kc, cap = m->cap, ccap = m->ccap, W = P.width, Hh = P.height;
  const size_t npx = m->npx;
  // ---- every frame is checked before anything is written or launched
  std::vector<uint8_t> seen(m->max_seq, 0);
  std::vector<uint8_t> new_local(n, 0);
  int total_imu = 0, max_local = 0;
  for (int i = 0; i < n; i++) {
    const int s = slots[i];
    if (s < 0 || s >= m->max_seq || seen[s]) {
      set_error("vieo_track_frames: frame %d: slot %d is out of range (0..%d) or appears twice", i, s, m->max_seq - 1);
      return VIEO_E_INVALID;
    }
    seen[s] = 1;
    const vieo_track_input* I = in + i;
    if (I->stride < W || I->n_imu < 0 || (I->n_imu > 0 && !I->imu) || I->n_last < 0 ||
        (I->n_last > 0 && (!I->last_points || !I->last_track_depth)) || I->n_local < 0 || (I->n_local > 0 && !I->local_alias) ||
        !I->left || !I->right) {
      set_error("vieo_track_frames: slot %d: invalid input (stride, counts, null arrays or images)", s);
      return VIEO_E_INVALID;
    }
    if (I->next_left || I->next_right || I->next_imu || I->use_prefetched || I->next_images[0] || I->next_images[1] ||
        I->next_images[2] || I->next_images[3]) {
      set_error("vieo_track_frames: slot %d: frame pipelining (next_* / use_prefetched) is not offered here", s);
      return VIEO_E_INVALID;
    }
    if (I->n_last > kc || I->n_local > ccap || I->n_imu > m->imu_cap) {
      set_error("vieo_track_frames: slot %d: %d last-frame points / %d local points / %d IMU samples exceed the capacities "
                "%d / %d / %d", s, I->n_last, I->n_local, I->n_imu, kc, ccap, m->imu_cap);
      return VIEO_E_CAPACITY;
    }
    new_local[i] = I->n_local > 0 && (I->local_version != m->local_version[s] || I->n_local != m->n_local_dev[s]);
    if (new_local[i] && (!I->local_points || !I->local_desc)) {
      set_error("vieo_track_frames: slot %d: a changed local map needs local_points and local_desc", s);
      return VIEO_E_INVALID;
    }
    total_imu += m->vision ? 0 : I->n_imu;
    max_local = std::max(max_local, (int)I->n_local);
  }
  int rc = require_device();
  if (rc != VIEO_OK) return rc;
  const auto t_enter = std::chrono::steady_clock::now();
  const MultiLayout L = multi_layout(m, n);
  // ---- the upload block
  uint8_t* H = m->h_up;
  vieo_sbp_camera* cam = (vieo_sbp_camera*)(H + L.u_cam);
  vieo_navstate* nref = (vieo_navstate*)(H + L.u_nref);
  vieo_navstate* nlast = (vieo_navstate*)(H + L.u_nlast);
  double *ti = (double*)(H + L.u_ti), *tj = (double*)(H + L.u_tj), *bg = (double*)(H + L.u_bg), *ba = (double*)(H + L.u_ba);
  int32_t *first = (int32_t*)(H + L.u_first), *nl = (int32_t*)(H + L.u_nl), *nloc = (int32_t*)(H + L.u_nloc);
  int32_t* pslot = (int32_t*)(H + L.u_slot);
  vieo_imu_sample* samples = (vieo_imu_sample*)(H + L.u_imu);
  first[0] = 0;
  for (int i = 0; i < n; i++) {
    const vieo_track_input* I = in + i;
    const int s = slots[i];
    cam[i] = m->cam0;
    cam[i].th = P.th_last;
    for (int which = 0; which < 2; which++) {
      uint8_t* dst = H + (which ? L.u_f2 : L.u_f1) + (size_t)i * m->fstride;
      vieo_vio_frame f = which ? m->f2_0 : m->f1_0;
      f.nav_last = I->nav_ref;
      f.dt_frames = I->t_cur - I->t_ref;
      f.last_has_prior = I->nav_prior && I->H_prior ? 1 : 0;
      if (f.last_has_prior) f.nav_prior = *I->nav_prior, memcpy(f.H_prior, I->H_prior, sizeof(f.H_prior));
      f.base.n_obs = 0, f.base.obs_begin = 0;
      memcpy(dst, &f, m->fstride);  // (vision-only: the leading vieo_pose_frame)
    }
    nref[i] = I->nav_ref, nlast[i] = I->nav_last;
    ti[i] = I->t_ref, tj[i] = I->t_cur;
    for (int k = 0; k < 3; k++) bg[3 * i + k] = I->nav_ref.bg[k], ba[3 * i + k] = I->nav_ref.ba[k];
    const int ni = m->vision ? 0 : I->n_imu;
    if (ni) memcpy(samples + first[i], I->imu, (size_t)ni * sizeof(vieo_imu_sample));
    first[i + 1] = first[i] + ni;
    nl[i] = I->n_last, nloc[i] = I->n_local, pslot[i] = s;
    if (I->n_last) {
      memcpy(H + L.u_pts + (size_t)i * kc * sizeof(vieo_last_frame_point), I->last_points,
             (size_t)I->n_last * sizeof(vieo_last_frame_point));
      float* xyz = (float*)(H + L.u_xyz) + (size_t)i * kc * 3;
      for (int k = 0; k < I->n_last; k++) {
        const float* X = I->last_points[k].Xw;
        xyz[3 * k] = X[0], xyz[3 * k + 1] = X[1], xyz[3 * k + 2] = X[2];
      }
      memcpy((float*)(H + L.u_dep) + (size_t)i * kc, I->last_track_depth, (size_t)I->n_last * 4);
    }
    if (I->n_local) memcpy((int32_t*)(H + L.u_alias) + (size_t)i * ccap, I->local_alias, (size_t)I->n_local * 4);
    // the images into the slot's pinned planes (nothing to do when the caller decoded them there)
    const uint8_t* src[2] = {I->left, I->right};
    for (int c = 0; c < 2; c++) {
      uint8_t* dst = m->h_img + ((size_t)s * 2 + c) * npx;
      if (src[c] == dst) continue;
      if (I->stride == W)
        memcpy(dst, src[c], npx);
      else
        for (int y = 0; y < Hh; y++) memcpy(dst + (size_t)y * W, src[c] + (size_t)y * I->stride, W);
    }
    if (new_local[i]) {
      const int nc = I->n_local;
      memcpy(m->h_loc + m->l_pts + (size_t)s * ccap * sizeof(vieo_frustum_point), I->local_points, (size_t)nc * sizeof(vieo_frustum_point));
      memcpy(m->h_loc + m->l_desc + (size_t)s * ccap * 32, I->local_desc, (size_t)nc * 32);
      float* xyz = (float*)(m->h_loc + m->l_xyz) + (size_t)s * ccap * 3;
      for (int k = 0; k < nc; k++) {
        const float* X = I->local_points[k].Xw;
        xyz[3 * k] = X[0], xyz[3 * k + 1] = X[1], xyz[3 * k + 2] = X[2];
      }
    }
  }
  // ---- one copy up (+ the images, + the local maps that changed), the chain, the copies back
  hipStream_t st = m->st, sb = m->st_imu;
  uint8_t *U = m->d_up, *O = m->d_out, *Wk = m->d_work;
#define MTRK_HIP(expr)                                                                      \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) {                                                                 \
      vieo::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
      return multi_fail(m, VIEO_E_HIP);                                                     \
    }                                                                                       \
  } while (0)
  MTRK_HIP(hipEventRecord(m->ev_t0, st));
  MTRK_HIP(hipMemcpyAsync(U, H, L.u_imu + (size_t)total_imu * sizeof(vieo_imu_sample), hipMemcpyHostToDevice, st));
  MTRK_HIP(hipEventRecord(m->ev_up, st));
  // (the unwritten last word of a vieo_vio_result stays zero, as in vieo_tracker's download block)
  MTRK_HIP(hipMemsetAsync(O + L.q_r1, 0, 2 * (size_t)n * m->rstride, st));
  for (int i = 0; i < n;) {  // the planes of runs of consecutive slots in one copy each
    int j = i + 1;
    while (j < n && slots[j] == slots[j - 1] + 1) j++;
    MTRK_HIP(hipMemcpyAsync(m->d_img + (size_t)i * 2 * npx, m->h_img + (size_t)slots[i] * 2 * npx, (size_t)(j - i) * 2 * npx,
                            hipMemcpyHostToDevice, st));
    i = j;
  }
  vieo_keypoint* d_kp = (vieo_keypoint*)(Wk + m->w_kp);
  uint8_t* d_desc = Wk + m->w_desc;
  int32_t* d_cnt = (int32_t*)(O + L.q_cnt);
  if ((rc = vieo_orb_extract_batch_device(m->ext, m->d_img, 2 * n, W, Hh, W, npx, nullptr, d_kp, d_desc, cap, d_cnt)) != VIEO_OK)
    return multi_fail(m, rc);
  // The second stream (handed over behind the extraction's launches, the head of the critical path): the local maps
  // that changed, the pre-integrations, the predictions and point tables, the first search's queries
  MTRK_HIP(hipStreamWaitEvent(sb, m->ev_up, 0));
  for (int i = 0; i < n; i++) {
    if (!new_local[i]) continue;
    const int s = slots[i], nc = in[i].n_local;
    const size_t op = m->l_pts + (size_t)s * ccap * sizeof(vieo_frustum_point), od = m->l_desc + (size_t)s * ccap * 32;
    const size_t ox = m->l_xyz + (size_t)s * ccap * 12;
    MTRK_HIP(hipMemcpyAsync(m->d_loc + op, m->h_loc + op, (size_t)nc * sizeof(vieo_frustum_point), hipMemcpyHostToDevice, sb));
    MTRK_HIP(hipMemcpyAsync(m->d_loc + od, m->h_loc + od, (size_t)nc * 32, hipMemcpyHostToDevice, sb));
    MTRK_HIP(hipMemcpyAsync(m->d_loc + ox, m->h_loc + ox, (size_t)nc * 12, hipMemcpyHostToDevice, sb));
  }
  const MultiTables tables{(const float*)(U + L.u_xyz), (const float*)(U + L.u_dep), (const float*)(m->d_loc + m->l_xyz),
                           (float*)(Wk + m->w_xyz), (float*)(Wk + m->w_dep), (const int32_t*)(U + L.u_nl),
                           (const int32_t*)(U + L.u_nloc), (const int32_t*)(U + L.u_slot), kc, ccap, m->pcap};
  if (!m->vision) {
    if ((rc = vieo_imu_preintegrate_batch_device((const vieo_imu_noise*)m->d_const, (const vieo_imu_sample*)(U + L.u_imu),
                                                 (const int32_t*)(U + L.u_first), (const double*)(U + L.u_ti),
                                                 (const double*)(U + L.u_tj), (const double*)(U + L.u_bg), (const double*)(U + L.u_ba),
                                                 n, (vieo_imu_preint*)(Wk + m->w_pre), (double*)(Wk + m->w_prv),
                                                 (int32_t*)(Wk + m->w_pst), sb)) != VIEO_OK)
      return multi_fail(m, rc);
    hipLaunchKernelGGL(k_track_predict_multi, dim3(1 + kTableBlocks, n), dim3(64), 0, sb, (const vieo_navstate*)(U + L.u_nref),
                       (const vieo_navstate*)(U + L.u_nlast), (vieo_vio_frame*)(U + L.u_f1), (vieo_vio_frame*)(U + L.u_f2),
                       (vieo_sbp_camera*)(U + L.u_cam), (vieo_navstate*)(O + L.q_nav), (vieo_imu_preint*)(O + L.q_imu),
                       (double*)(O + L.q_sig), (int32_t*)(O + L.q_pst), (const vieo_imu_preint*)(Wk + m->w_pre),
                       (const double*)(Wk + m->w_prv), (const int32_t*)(Wk + m->w_pst), (double*)(Wk + m->w_bias), tables);
  } else {
    hipLaunchKernelGGL(k_track_set_pose_multi, dim3(1 + kTableBlocks, n), dim3(64), 0, sb, (const vieo_navstate*)(U + L.u_nref),
                       (const vieo_navstate*)(U + L.u_nlast), (vieo_pose_frame*)(U + L.u_f1), (vieo_pose_frame*)(U + L.u_f2),
                       (vieo_sbp_camera*)(U + L.u_cam), (vieo_navstate*)(O + L.q_nav), (int32_t*)(O + L.q_pst), tables);
  }
  MTRK_HIP(hipGetLastError());
  if ((rc = vieo_sbp_project_last_frame_batch_device((const vieo_last_frame_point*)(U + L.u_pts), (const int32_t*)(U + L.u_nl), kc,
                                                     n, (const vieo_sbp_camera*)(U + L.u_cam), (vieo_proj_query*)(Wk + m->w_q1),
                                                     sb)) != VIEO_OK)
    return multi_fail(m, rc);
  MTRK_HIP(hipEventRecord(m->ev_imu, sb));
  // ComputeStereoMatches of the n frames
  if ((rc = vieo_stereo_match_rectified_batch_device(m->ext, n, d_kp, d_desc, d_cnt, cap, P.baseline, P.bf, (float*)(O + L.q_ur),
                                                     (float*)(O + L.q_dp))) != VIEO_OK)
    return multi_fail(m, rc);
  MTRK_HIP(hipEventRecord(m->ev_ext, st));
  // the left images' keys / descriptors back on the second stream, beside the tail
  MTRK_HIP(hipStreamWaitEvent(sb, m->ev_ext, 0));
  MTRK_HIP(hipMemcpy2DAsync(m->h_out + L.q_kp, (size_t)cap * sizeof(vieo_keypoint), d_kp, 2 * (size_t)cap * sizeof(vieo_keypoint),
                            (size_t)cap * sizeof(vieo_keypoint), n, hipMemcpyDeviceToHost, sb));
  MTRK_HIP(hipMemcpy2DAsync(m->h_out + L.q_desc, (size_t)cap * 32, d_desc, 2 * (size_t)cap * 32, (size_t)cap * 32, n,
                            hipMemcpyDeviceToHost, sb));
  MTRK_HIP(hipEventRecord(m->ev_kd, sb));
  MTRK_HIP(hipStreamWaitEvent(st, m->ev_imu, 0));
  if ((rc = multi_tail(m, L, n, max_local, true)) != VIEO_OK) return multi_fail(m, rc);
  MTRK_HIP(hipStreamWaitEvent(st, m->ev_kd, 0));
  MTRK_HIP(hipEventRecord(m->ev_t1, st));
  MTRK_HIP(hipStreamSynchronize(st));
  const int32_t* nm1 = (const int32_t*)(m->h_out + L.q_nm1);
  const int32_t* pst = (const int32_t*)(m->h_out + L.q_pst);
  const vieo_imu_preint* imu = (const vieo_imu_preint*)(m->h_out + L.q_imu);
  std::vector<uint8_t> widened(n, 0);
  int n_wide = 0;
  for (int i = 0; i < n; i++) {
    const bool pre_ok = m->vision || (pst[i] == 0 && imu[i].dt != 0);
    if (nm1[i] < 20 && pre_ok) {
      // Tracking.cc:301-309 / :1869-1876: the wider window for this frame; the tail runs again over all frames
      widened[i] = 1, n_wide++;
      cam[i].th = 2 * P.th_last;
      MTRK_HIP(hipMemcpyAsync(U + L.u_cam + (size_t)i * sizeof(vieo_sbp_camera) + offsetof(vieo_sbp_camera, th), &cam[i].th, 4,
                              hipMemcpyHostToDevice, st));
    }
  }
  if (n_wide) {
    if ((rc = multi_tail(m, L, n, max_local, false)) != VIEO_OK) return multi_fail(m, rc);
    MTRK_HIP(hipEventRecord(m->ev_t1, st));
    MTRK_HIP(hipStreamSynchronize(st));
  }
#undef MTRK_HIP
  for (int i = 0; i < n; i++)
    if (new_local[i]) m->local_version[slots[i]] = in[i].local_version, m->n_local_dev[slots[i]] = in[i].n_local;
  float ms_gpu = 0;
  (void)hipEventElapsedTime(&ms_gpu, m->ev_t0, m->ev_t1);
  const float ms_host = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_enter).count();
  const uint8_t* Q = m->h_out;
  const int32_t* cnt = (const int32_t*)(Q + L.q_cnt);
  for (int i = 0; i < n; i++) {
    vieo_track_output* o = out + i;
    memset(o, 0, sizeof(*o));
    const bool pre_ok = m->vision || (pst[i] == 0 && imu[i].dt != 0);
    o->preint_status = pst[i];
    o->status = !pre_ok ? VIEO_TRACK_PREINT_FAILED : (nm1[i] < (m->vision ? 20 : 10) ? VIEO_TRACK_LOST : VIEO_TRACK_OK);
    o->n_keys = std::min(cnt[4 * i], cap);
    o->cam_first[1] = o->n_keys;
    o->key_cap = kc;
    o->keys = (const vieo_keypoint*)(Q + L.q_kp) + (size_t)i * cap, o->desc = Q + L.q_desc + (size_t)i * cap * 32;
    o->uright = (const float*)(Q + L.q_ur) + (size_t)i * kc, o->depth = (const float*)(Q + L.q_dp) + (size_t)i * kc;
    o->point_ref = (const int32_t*)(Q + L.q_mpref) + (size_t)i * kc, o->outlier = Q + L.q_outl + (size_t)i * kc;
    o->local_track_depth = (const float*)(Q + L.q_cdep) + (size_t)i * ccap;
    o->n_matches_last = nm1[i], o->n_matches_local = ((const int32_t*)(Q + L.q_nm2))[i], o->widened = widened[i];
    o->nav_pred = ((const vieo_navstate*)(Q + L.q_nav))[i];
    if (!m->vision) o->imu = imu[i];
    memcpy(&o->first, Q + L.q_r1 + (size_t)i * m->rstride, m->rstride);  // (vision-only: .base, the rest stays zero)
    memcpy(&o->second, Q + L.q_r2 + (size_t)i * m->rstride, m->rstride);
    o->ms_gpu = ms_gpu, o->ms_host = ms_host;
  }
  return VIEO_OK;
}

}  // extern "C"
