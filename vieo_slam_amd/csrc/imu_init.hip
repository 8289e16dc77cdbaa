// imu_init.hip -- IMUInitialization::TryInitVIO (reference src/Odom/IMUInitialization.cpp:1068-1480, the default path) for
// a batch of sequences in one call (vieo_imu_init).  One arena, one pinned copy up, one chain of launches on one stream
//   [k_imu_preint: the stored pre-integrations, when the caller passes none]   (a pre-integration pass: ii_preint_pass)
//   k_imu_init_gyro     one wavefront per sequence: the Gauss-Newton step for bg*, written into the result and into the
//                       per-interval bias table the next launch reads
//   k_imu_preint        every interval of every sequence with (bg*, 0)
//   k_imu_init_solve    one wavefront per sequence: the rows of [A | B] in LDS, the Jacobi SVD, RwI, the rows of [C | D]
//                       in the same LDS, the second SVD, the whole result record; ba* into the bias table
//   k_imu_preint        every interval with (bg*, ba*), straight into the output
//   k_imu_init_apply    flat over (sequence, key frame) and (sequence, point): scaled Tcw, NavState, velocity, the
//                       set / not-set flag, scaled points; sequences whose gate is closed or whose status is not OK get zeros
// one copy back, one synchronisation.  The pre-integration kernel is imu_preint.hip's, untouched.  A fixed lane <-> row
// map and the fixed DPP tree make a sequence's result independent of its neighbours in the batch and of the run.  The lane
// functions are imu_init_device.h's.
#include "common.h"
#include "imu_init_device.h"
#include "wave_ops.h"

namespace vieo {
namespace {

struct WaveLanes {
  int lane;
  template <int N, class F>
  __device__ __forceinline__ void run(F f, double* out) {
    double part[N];
    f(lane, 64, part);
#pragma unroll
    for (int i = 0; i < N; i++) out[i] = wave_sum_f64(part[i]);
  }
  __device__ __forceinline__ void sync() { __syncthreads(); }  // (one wavefront per workgroup)
};

__device__ __forceinline__ IiSeq ii_view(const vieo_imu_init_seq& q, const double* Twc, const vieo_imu_preint* pre,
                                         const double* prv) {
  IiSeq S;
  S.Twc = Twc + 12 * (size_t)q.kf_first, S.pre = pre + q.kf_first, S.prv = prv ? prv + 81 * (size_t)q.kf_first : nullptr;
  S.n = q.n_kf_init, S.G = q.ref_g;
  for (int i = 0; i < 9; i++) S.Rcb[i] = q.Rcb[i];
  for (int i = 0; i < 3; i++) S.pcb[i] = q.pcb[i];
  return S;
}

__global__ __launch_bounds__(64) void k_imu_init_gyro(const vieo_imu_init_seq* __restrict__ seqs,
                                                      const double* __restrict__ Twc,
                                                      const vieo_imu_preint* __restrict__ pre,
                                                      const double* __restrict__ prv, double* __restrict__ bg_tab,
                                                      vieo_imu_init_result* __restrict__ results) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const vieo_imu_init_seq q = seqs[b];
  double bg[3] = {0, 0, 0};
  int n_eq = 0;
  if (q.n_kf_init >= 4) {  // (uniform)
    const IiSeq S = ii_view(q, Twc, pre, prv);
    WaveLanes L{lane};
    ii_gyro_step(L, S, bg, &n_eq);
  }
  for (int k = lane; k < q.n_kf; k += 64)
    for (int j = 0; j < 3; j++) bg_tab[3 * (size_t)(q.kf_first + k) + j] = bg[j];
  if (lane == 0) {
    vieo_imu_init_result R;
    memset(&R, 0, sizeof(R));
    R.status = q.n_kf_init >= 4 ? VIEO_IMU_INIT_OK : VIEO_IMU_INIT_FEW_KF;
    R.n_eq_gyro = n_eq;
    for (int j = 0; j < 3; j++) R.bg[j] = bg[j];
    results[b] = R;
  }
}

__global__ __launch_bounds__(64) void k_imu_init_solve(const vieo_imu_init_seq* __restrict__ seqs,
                                                       const double* __restrict__ Twc,
                                                       const vieo_imu_preint* __restrict__ pre,
                                                       double* __restrict__ ba_tab,
                                                       vieo_imu_init_result* __restrict__ results) {
  extern __shared__ __attribute__((aligned(16))) double s_rows[];  // 7 columns of 3 (n_kf_init - 2) rows
  const int b = blockIdx.x, lane = threadIdx.x;
  const vieo_imu_init_seq q = seqs[b];
  vieo_imu_init_result R = results[b];
  if (R.status != VIEO_IMU_INIT_OK) return;  // FEW_KF (uniform)
  const IiSeq S = ii_view(q, Twc, pre, nullptr);
  WaveLanes L{lane};
  ii_solve(L, S, s_rows, 3 * (q.n_kf_init - 2), R);
  R.inited = R.status == VIEO_IMU_INIT_OK && q.apply != 0;
  if (R.status == VIEO_IMU_INIT_OK)
    for (int k = lane; k < q.n_kf; k += 64)
      for (int j = 0; j < 3; j++) ba_tab[3 * (size_t)(q.kf_first + k) + j] = R.ba[j];
  if (lane == 0) results[b] = R;
}

// blockIdx.y = the sequence; blockIdx.x < kf_blocks: its key frames, one lane each; the blocks behind: its points
__global__ __launch_bounds__(64) void k_imu_init_apply(const vieo_imu_init_seq* __restrict__ seqs, int kf_blocks,
                                                       const double* __restrict__ Twc,
                                                       const vieo_imu_init_result* __restrict__ results,
                                                       const vieo_imu_init_point* __restrict__ points,
                                                       vieo_imu_preint* __restrict__ pre, double* __restrict__ prv,
                                                       double* __restrict__ Tcw_out, vieo_navstate* __restrict__ nav_out,
                                                       int32_t* __restrict__ nav_set,
                                                       vieo_imu_init_point* __restrict__ points_out) {
  const int b = blockIdx.y;
  const vieo_imu_init_seq& q = seqs[b];
  const vieo_imu_init_result& R = results[b];
  const bool inited = R.inited != 0;
  if ((int)blockIdx.x >= kf_blocks) {
    const int i = ((int)blockIdx.x - kf_blocks) * 64 + threadIdx.x;
    if (i >= q.n_points || !inited) return;  // (the outputs were cleared before the chain)
    const float s = (float)R.s;  // MapPoint::UpdateScale((float)scale)
    const vieo_imu_init_point p = points[q.point_first + i];
    vieo_imu_init_point o;
    for (int k = 0; k < 3; k++) o.pos[k] = p.pos[k] * s;
    o.max_dist = p.max_dist * s, o.min_dist = p.min_dist * s;
    points_out[q.point_first + i] = o;
    return;
  }
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= q.n_kf) return;
  const size_t g = (size_t)q.kf_first + k;
  if (!inited) {  // the last pre-integration pass wrote this sequence's intervals too
    double* P = (double*)(pre + g);
    for (int i = 0; i < (int)(sizeof(vieo_imu_preint) / 8); i++) P[i] = 0;
    for (int i = 0; i < 81; i++) prv[81 * g + i] = 0;
    return;
  }
  const double s = R.s;
  const double* T = Twc + 12 * g;
  ii_scaled_Tcw(T, s, Tcw_out + 12 * g);
  const bool last = k == q.n_kf - 1;
  const vieo_imu_preint& M = pre[last ? g : g + 1];  // the interval this key frame's velocity comes from
  const double dt = M.dt;
  if (dt == 0) return;  // the reference's `continue`: the pose is scaled, the NavState is not set
  vieo_navstate ns;
  double Rwb[9];
  ii_nav_pose(T, q.Rcb, q.pcb, s, ns.p, ns.q, Rwb);
  for (int j = 0; j < 3; j++) ns.bg[j] = R.bg[j], ns.ba[j] = R.ba[j], ns.dbg[j] = 0, ns.dba[j] = 0;
  if (!last)
    ii_velocity(T, T + 12, q.Rcb, q.pcb, s, R.gw, dt, M.pij, ns.v);
  else {
    // v = v_prev + gw dt + Rwb_prev dv: the predecessor's velocity is recomputed here instead of waited for (it is set:
    // its `continue` is this key frame's dt == 0)
    double vp[3], Rp[9], Rpb[9], r[3];
    ii_velocity(T - 12, T, q.Rcb, q.pcb, s, R.gw, dt, M.pij, vp);
    ii_Rwc(T - 12, Rp);
    mm3(Rp, q.Rcb, Rpb);
    mv3(Rpb, M.vij, r);
    for (int j = 0; j < 3; j++) ns.v[j] = vp[j] + R.gw[j] * dt + r[j];
  }
  nav_out[g] = ns;
  nav_set[g] = 1;
}

const int kIiLdsMax = 3 * (VIEO_IMU_INIT_MAX_KF - 2) * 7 * 8;  // 85 680 bytes

// One pre-integration pass over all intervals.  vieo_imu_preintegrate_batch_device gives every interval a wavefront below
// 1024 intervals and a lane from there on (the same bytes either way); an interval here is a key-frame interval of tens of
// samples, a serial recursion, and the lane form leaves a pass of 1920 intervals at 11 ms on 30 wavefronts.  So the pass
// goes out in slices of 1023: 0.4 ms each, every interval on a wavefront of its own.
const int kIiPreintSlice = 1023;
int ii_preint_pass(const vieo_imu_noise* noise, const vieo_imu_sample* samples, const int32_t* first, const double* ti,
                   const double* tj, const double* bg, const double* ba, int n, vieo_imu_preint* out, double* prv,
                   int32_t* status, hipStream_t st) {
  for (int k = 0; k < n; k += kIiPreintSlice) {
    const int m = n - k < kIiPreintSlice ? n - k : kIiPreintSlice;
    const int rc = vieo_imu_preintegrate_batch_device(noise, samples, first + k, ti + k, tj + k, bg + 3 * (size_t)k,
                                                      ba + 3 * (size_t)k, m, out + k, prv + 81 * (size_t)k, status + k, st);
    if (rc != VIEO_OK) return rc;
  }
  return VIEO_OK;
}

}  // namespace
}  // namespace vieo

using namespace vieo;

extern "C" int vieo_imu_init(const vieo_imu_init_seq* seqs, int n_seq, int total_kf, const double* h_Twc, const double* h_t,
                             const vieo_imu_noise* noise, const vieo_imu_sample* h_samples, const int32_t* h_first,
                             const vieo_imu_preint* h_preint, const double* h_preint_sigma_prv,
                             const vieo_imu_init_point* h_points, int total_points, vieo_imu_init_result* h_results,
                             double* h_Tcw_out, vieo_navstate* h_nav_out, int32_t* h_nav_set,
                             vieo_imu_preint* h_preint_out, double* h_sigma_prv_out, vieo_imu_init_point* h_points_out) {
  if (!seqs || !h_Twc || !h_t || !noise || !h_first || !h_results || !h_Tcw_out || !h_nav_out || !h_nav_set ||
      !h_preint_out || !h_sigma_prv_out || (!h_preint) != (!h_preint_sigma_prv) || total_points < 0 ||
      (total_points > 0 && (!h_points || !h_points_out))) {
    set_error("vieo_imu_init: a null pointer, or only one of h_preint / h_preint_sigma_prv");
    return VIEO_E_INVALID;
  }
  if (n_seq < 1 || n_seq > VIEO_IMU_INIT_MAX_SEQ || total_kf < 1) {
    set_error("vieo_imu_init: n_seq = %d (1..%d), total_kf = %d", n_seq, VIEO_IMU_INIT_MAX_SEQ, total_kf);
    return VIEO_E_INVALID;
  }
  int max_kf = 0, max_init = 0, max_points = 0;
  for (int b = 0; b < n_seq; b++) {
    const vieo_imu_init_seq& q = seqs[b];
    if (q.n_kf < 1 || q.n_kf > VIEO_IMU_INIT_MAX_KF || q.n_kf_init < 0 || q.n_kf_init > q.n_kf || q.kf_first < 0 ||
        q.kf_first > total_kf - q.n_kf || q.n_points < 0 || q.point_first < 0 || q.point_first > total_points - q.n_points) {
      set_error("vieo_imu_init: sequence %d: n_kf = %d (1..%d), n_kf_init = %d, key frames [%d, +%d) of %d, points [%d, +%d) of %d",
                b, q.n_kf, VIEO_IMU_INIT_MAX_KF, q.n_kf_init, q.kf_first, q.n_kf, total_kf, q.point_first, q.n_points,
                total_points);
      return VIEO_E_INVALID;
    }
    for (int c = 0; c < b; c++) {
      const vieo_imu_init_seq& o = seqs[c];
      const bool kf_apart = q.kf_first + q.n_kf <= o.kf_first || o.kf_first + o.n_kf <= q.kf_first;
      const bool pt_apart = q.n_points == 0 || o.n_points == 0 || q.point_first + q.n_points <= o.point_first ||
                            o.point_first + o.n_points <= q.point_first;
      if (!kf_apart || !pt_apart) {
        set_error("vieo_imu_init: sequences %d and %d share key frames or points", c, b);
        return VIEO_E_INVALID;
      }
    }
    max_kf = q.n_kf > max_kf ? q.n_kf : max_kf, max_init = q.n_kf_init > max_init ? q.n_kf_init : max_init;
    max_points = q.n_points > max_points ? q.n_points : max_points;
  }
  if (h_first[0] < 0) {
    set_error("vieo_imu_init: h_first[0] < 0");
    return VIEO_E_INVALID;
  }
  for (int k = 0; k < total_kf; k++)
    if (h_first[k + 1] < h_first[k]) {
      set_error("vieo_imu_init: h_first descends at %d", k);
      return VIEO_E_INVALID;
    }
  const int total_samples = h_first[total_kf];
  if (total_samples > 0 && !h_samples) {
    set_error("vieo_imu_init: samples listed, h_samples == NULL");
    return VIEO_E_INVALID;
  }
  int rc = require_device();
  if (rc != VIEO_OK) return rc;

  const size_t n = (size_t)total_kf, np = (size_t)total_points;
  static thread_local Staging S;
  S.reset();
  const size_t o_seqs = S.in(seqs, sizeof(vieo_imu_init_seq) * n_seq);
  const size_t o_Twc = S.in(h_Twc, 96 * n);
  const size_t o_noise = S.in(noise, sizeof(vieo_imu_noise));
  const size_t o_first = S.in(h_first, 4 * (n + 1));
  const size_t o_samples = S.in(h_samples, sizeof(vieo_imu_sample) * (size_t)total_samples);
  const size_t o_pre0 = S.in(h_preint, h_preint ? sizeof(vieo_imu_preint) * n : 0);
  const size_t o_prv0 = S.in(h_preint_sigma_prv, h_preint ? 648 * n : 0);
  const size_t o_points = S.in(h_points, sizeof(vieo_imu_init_point) * np);
  const size_t o_ti = S.in(nullptr, 8 * n), o_tj = S.in(nullptr, 8 * n);  // written below
  const size_t o_res = S.out(sizeof(vieo_imu_init_result) * n_seq);
  const size_t o_Tcw = S.out(96 * n), o_nav = S.out(sizeof(vieo_navstate) * n), o_set = S.out(4 * n);
  const size_t o_pre3 = S.out(sizeof(vieo_imu_preint) * n), o_prv3 = S.out(648 * n);
  const size_t o_pts = S.out(sizeof(vieo_imu_init_point) * np);
  const size_t o_end = S.used;
  const size_t o_bg = S.scratch(24 * n), o_ba0 = S.scratch(24 * n), o_ba = S.scratch(24 * n), o_st = S.scratch(4 * n);
  const size_t o_pre1 = S.scratch(sizeof(vieo_imu_preint) * n), o_prv1 = S.scratch(648 * n);
  const size_t o_pre0s = S.scratch(h_preint ? 0 : sizeof(vieo_imu_preint) * n), o_prv0s = S.scratch(h_preint ? 0 : 648 * n);
  if ((rc = S.alloc()) != VIEO_OK) return rc;
  {  // interval k = (key frame k - 1) -> key frame k; a sequence's key frame 0 owns an interval without samples
    double *ti = S.hw<double>(o_ti), *tj = S.hw<double>(o_tj);
    for (size_t k = 0; k < n; k++) ti[k] = tj[k] = h_t[k];
    for (int b = 0; b < n_seq; b++)
      for (int k = 1; k < seqs[b].n_kf; k++) ti[seqs[b].kf_first + k] = h_t[seqs[b].kf_first + k - 1];
  }
  hipStream_t st = 0;
  if ((rc = S.upload(st)) != VIEO_OK) return rc;
  VIEO_HIP_CHECK(hipMemsetAsync(S.d<uint8_t>(o_res), 0, o_end - o_res, st));
  VIEO_HIP_CHECK(hipMemsetAsync(S.d<uint8_t>(o_bg), 0, o_st - o_bg, st));  // bg, the zero ba of pass 2, ba
  const vieo_imu_init_seq* d_seqs = S.d<vieo_imu_init_seq>(o_seqs);
  const double* d_Twc = S.d<double>(o_Twc);
  const vieo_imu_noise* d_noise = S.d<vieo_imu_noise>(o_noise);
  const vieo_imu_sample* d_samples = S.d<vieo_imu_sample>(o_samples);
  const int32_t* d_first = S.d<int32_t>(o_first);
  const double *d_ti = S.d<double>(o_ti), *d_tj = S.d<double>(o_tj);
  double *d_bg = S.d<double>(o_bg), *d_ba0 = S.d<double>(o_ba0), *d_ba = S.d<double>(o_ba);
  int32_t* d_st = S.d<int32_t>(o_st);
  vieo_imu_init_result* d_res = S.d<vieo_imu_init_result>(o_res);
  const vieo_imu_preint* d_pre0 = S.d<vieo_imu_preint>(h_preint ? o_pre0 : o_pre0s);
  const double* d_prv0 = S.d<double>(h_preint ? o_prv0 : o_prv0s);
  if (!h_preint &&
      (rc = ii_preint_pass(d_noise, d_samples, d_first, d_ti, d_tj, d_ba0, d_ba0, total_kf, S.d<vieo_imu_preint>(o_pre0s),
                           S.d<double>(o_prv0s), d_st, st)) != VIEO_OK)
    return rc;
  hipLaunchKernelGGL(k_imu_init_gyro, dim3(n_seq), dim3(64), 0, st, d_seqs, d_Twc, d_pre0, d_prv0, d_bg, d_res);
  VIEO_HIP_CHECK(hipGetLastError());
  if ((rc = ii_preint_pass(d_noise, d_samples, d_first, d_ti, d_tj, d_bg, d_ba0, total_kf, S.d<vieo_imu_preint>(o_pre1),
                           S.d<double>(o_prv1), d_st, st)) != VIEO_OK)
    return rc;
  const int lds = max_init > 2 ? 3 * (max_init - 2) * 7 * 8 : 8;
  VIEO_HIP_CHECK(hipFuncSetAttribute((const void*)k_imu_init_solve, hipFuncAttributeMaxDynamicSharedMemorySize, kIiLdsMax));
  hipLaunchKernelGGL(k_imu_init_solve, dim3(n_seq), dim3(64), lds, st, d_seqs, d_Twc, S.d<vieo_imu_preint>(o_pre1), d_ba, d_res);
  VIEO_HIP_CHECK(hipGetLastError());
  if ((rc = ii_preint_pass(d_noise, d_samples, d_first, d_ti, d_tj, d_bg, d_ba, total_kf, S.d<vieo_imu_preint>(o_pre3),
                           S.d<double>(o_prv3), d_st, st)) != VIEO_OK)
    return rc;
  const int kf_blocks = (max_kf + 63) / 64, pt_blocks = (max_points + 63) / 64;
  hipLaunchKernelGGL(k_imu_init_apply, dim3(kf_blocks + pt_blocks, n_seq), dim3(64), 0, st, d_seqs, kf_blocks, d_Twc, d_res,
                     S.d<vieo_imu_init_point>(o_points), S.d<vieo_imu_preint>(o_pre3), S.d<double>(o_prv3),
                     S.d<double>(o_Tcw), S.d<vieo_navstate>(o_nav), S.d<int32_t>(o_set), S.d<vieo_imu_init_point>(o_pts));
  VIEO_HIP_CHECK(hipGetLastError());
  if ((rc = S.download(o_res, o_end, st)) != VIEO_OK) return rc;
  memcpy(h_results, S.h(o_res), sizeof(vieo_imu_init_result) * n_seq);
  memcpy(h_Tcw_out, S.h(o_Tcw), 96 * n);
  memcpy(h_nav_out, S.h(o_nav), sizeof(vieo_navstate) * n);
  memcpy(h_nav_set, S.h(o_set), 4 * n);
  memcpy(h_preint_out, S.h(o_pre3), sizeof(vieo_imu_preint) * n);
  memcpy(h_sigma_prv_out, S.h(o_prv3), 648 * n);
  if (np) memcpy(h_points_out, S.h(o_pts), sizeof(vieo_imu_init_point) * np);
  return VIEO_OK;
}
