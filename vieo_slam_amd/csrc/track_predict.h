// track_predict.h -- the per-frame head of the one-call trackers, shared by tracker.hip (one frame per call) and
// tracker_multi.hip (one frame per live sequence, n per call): PredictNavStateByIMU / the vision-only pose set-up of one
// frame, and the copy of its point tables.  The kernels of both trackers call these bodies, so a frame's arithmetic is the
// same whichever tracker runs it.
#pragma once
#include "imu_device.h"

namespace vieo {

// The last frame's part of the tail's two point tables ([last frame's points | local candidates]: positions, track depths)
// comes up with the header; blocks 1.. of the prediction kernels move it in place (two copies and an event less to hand
// to the second stream per frame).
constexpr int kTableBlocks = 16;
struct TrkTables {
  const float *xyz_in, *dep_in;
  float *xyz_out, *dep_out;
};
__device__ __forceinline__ void track_fill_tables(const TrkTables& T, int n_last) {
  const int i0 = (blockIdx.x - 1) * 64 + threadIdx.x, step = kTableBlocks * 64;
  for (int i = i0; i < 3 * n_last; i += step) T.xyz_out[i] = T.xyz_in[i];
  for (int i = i0; i < n_last; i += step) T.dep_out[i] = T.dep_in[i];
}

// PredictNavStateByIMU (Tracking.cc:385-451) of one frame from its pre-integration in HBM; fills the two optimiser
// problems and the projection search's camera.  One wavefront; lane 0 does the (double) arithmetic, all lanes copy.
// s_nav: the workgroup's shared slot for the predicted state.
__device__ __forceinline__ void track_predict_frame(const vieo_navstate* nav_ref, const vieo_navstate* nav_last,
                                                    vieo_vio_frame* f1, vieo_vio_frame* f2, vieo_sbp_camera* cam,
                                                    vieo_navstate* nav_pred, vieo_imu_preint* imu_out, double* sigma_out,
                                                    int32_t* status_out, const vieo_imu_preint* pre, const double* sigma_prv,
                                                    const int32_t* status, double* next_bias, vieo_navstate& s_nav) {
  const int lane = threadIdx.x;
  const vieo_imu_preint& M = *pre;
  if (lane == 0) {
    vieo_navstate ns = *nav_ref;
    const double dt = M.dt;
    if (dt != 0) {
      const Qd q{ns.q[0], ns.q[1], ns.q[2], ns.q[3]};
      double Rwb[9], t0[3], t1[3], t2[3], r[3];
      q_to_R(q, Rwb);
      // p += v dt + g dt^2 / 2 + Rwb (pij + Jgp dbg + Jap dba)
      mv3(M.Jgp, ns.dbg, t0), mv3(M.Jap, ns.dba, t1);
      for (int k = 0; k < 3; k++) t2[k] = M.pij[k] + t0[k] + t1[k];
      mv3(Rwb, t2, r);
      double pn[3], vn[3];
      for (int k = 0; k < 3; k++) pn[k] = ns.p[k] + (ns.v[k] * dt + f1->gw[k] * (dt * dt / 2) + r[k]);
      mv3(M.Jgv, ns.dbg, t0), mv3(M.Jav, ns.dba, t1);
      for (int k = 0; k < 3; k++) t2[k] = M.vij[k] + t0[k] + t1[k];
      mv3(Rwb, t2, r);
      for (int k = 0; k < 3; k++) vn[k] = ns.v[k] + (f1->gw[k] * dt + r[k]);
      // Rwb *= Rij Exp(JgR dbg)
      double w[3], E[9], A[9], Rn[9];
      mv3(M.JgR, ns.dbg, w);
      q_to_R(so3_exp_q(w), E);
      mm3(M.Rij, E, A);
      mm3(Rwb, A, Rn);
      const Qd qn = R_to_q(Rn);
      for (int k = 0; k < 3; k++) ns.p[k] = pn[k], ns.v[k] = vn[k];
      ns.q[0] = qn.w, ns.q[1] = qn.x, ns.q[2] = qn.y, ns.q[3] = qn.z;
    }
    for (int k = 0; k < 3; k++) {  // bj_bar = bi_bar + dbi, also when the pre-integration failed (Tracking.cc:413-419)
      ns.bg[k] += ns.dbg[k], ns.ba[k] += ns.dba[k];
      ns.dbg[k] = 0, ns.dba[k] = 0;
    }
    s_nav = ns;
    // (bj_bar: the bias the NEXT frame's pre-integration runs with when this frame is its reference)
    for (int k = 0; k < 3; k++) next_bias[k] = ns.bg[k], next_bias[3 + k] = ns.ba[k];
    // Tcw = Tcb Twb^-1 of the predicted and of the last frame's state (UpdatePoseFromNS)
    for (int which = 0; which < 2; which++) {
      const vieo_navstate& n = which == 0 ? ns : *nav_last;
      const Qd q{n.q[0], n.q[1], n.q[2], n.q[3]};
      double Rwb[9];
      q_to_R(q, Rwb);
      const double* Rcb = f1->base.Rcb;
      double* T = which == 0 ? cam->Tcw_cur : cam->Tcw_last;
      for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++)
          T[r * 4 + c] = Rcb[r * 3] * Rwb[c * 3] + Rcb[r * 3 + 1] * Rwb[c * 3 + 1] + Rcb[r * 3 + 2] * Rwb[c * 3 + 2];
        T[r * 4 + 3] = f1->base.tcb[r] - (T[r * 4] * n.p[0] + T[r * 4 + 1] * n.p[1] + T[r * 4 + 2] * n.p[2]);
      }
    }
    *status_out = status[0];
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __syncthreads();
  const double* sn = (const double*)&s_nav;
  for (int i = lane; i < (int)(sizeof(vieo_navstate) / 8); i += 64) {
    ((double*)&f1->base.nav)[i] = sn[i], ((double*)&f2->base.nav)[i] = sn[i];
    ((double*)nav_pred)[i] = sn[i];
  }
  const double* sm = (const double*)pre;
  for (int i = lane; i < (int)(sizeof(vieo_imu_preint) / 8); i += 64) {
    ((double*)&f1->imu)[i] = sm[i], ((double*)&f2->imu)[i] = sm[i];
    ((double*)imu_out)[i] = sm[i];
  }
  for (int i = lane; i < 81; i += 64) sigma_out[i] = sigma_prv[i];
}

// The vision-only tracker's prediction comes from the host (mVelocity * mLastFrame.Tcw, Tracking.cc:1852): the two
// optimiser problems (vieo_pose_frame) start from it, the projection search gets Tcw of it and of the last frame.
// Rcb / tcb: the frames' extrinsics.  One wavefront.
__device__ __forceinline__ void track_set_pose_frame(const vieo_navstate* nav_ref, const vieo_navstate* nav_last,
                                                     const double* Rcb, const double* tcb, vieo_sbp_camera* cam,
                                                     vieo_navstate* f1_nav, vieo_navstate* f2_nav, vieo_navstate* nav_pred,
                                                     int32_t* status_out) {
  const int lane = threadIdx.x;
  if (lane < 2) {
    const vieo_navstate& n = lane == 0 ? *nav_ref : *nav_last;
    const Qd q{n.q[0], n.q[1], n.q[2], n.q[3]};
    double Rwb[9];
    q_to_R(q, Rwb);
    double* T = lane == 0 ? cam->Tcw_cur : cam->Tcw_last;
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++)
        T[r * 4 + c] = Rcb[r * 3] * Rwb[c * 3] + Rcb[r * 3 + 1] * Rwb[c * 3 + 1] + Rcb[r * 3 + 2] * Rwb[c * 3 + 2];
      T[r * 4 + 3] = tcb[r] - (T[r * 4] * n.p[0] + T[r * 4 + 1] * n.p[1] + T[r * 4 + 2] * n.p[2]);
    }
  }
  const double* sn = (const double*)nav_ref;
  for (int i = lane; i < (int)(sizeof(vieo_navstate) / 8); i += 64) {
    ((double*)f1_nav)[i] = sn[i], ((double*)f2_nav)[i] = sn[i];
    ((double*)nav_pred)[i] = sn[i];
  }
  if (lane == 0) *status_out = 0;
}

// per-key outlier flags of the second optimisation (mvbOutlier) and its observation count, one workgroup per frame;
// f2: vieo_vio_frame or vieo_pose_frame records, f2_stride bytes apart (both start with the vieo_pose_frame)
static __global__ void __launch_bounds__(256)
k_track_finish(const int32_t* __restrict__ obs_key, const uint8_t* __restrict__ outl, const uint8_t* __restrict__ f2,
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

// The tracker's second stream: the candidate among a few that runs beside main_stream (tracker.hip).  *ratio_out: what
// the kept stream measured.
hipError_t create_side_stream(hipStream_t* out, hipStream_t main_stream, float* ratio_out);

}  // namespace vieo
