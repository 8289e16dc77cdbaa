// track_chain.h -- the host code that tracker.hip (vieo_track_frame) and tracker_multi.hip (vieo_track_frames) share: the
// chain behind the prediction (track_run_chain over a TrackChain), the constants of a tracker's frames, the per-call
// record filling, the input checks, the decisions taken from a frame's results and the layout-free output fields.  The
// steps that differ stay with their owner: callables given to track_run_chain, or code around the call.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "common.h"
#include "track_predict.h"

namespace vieo {

static inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }
struct Layout {  // offsets of a block's arrays, each on a 256-byte boundary; o: the block's size so far
  size_t o = 0;
  size_t take(size_t bytes) { const size_t r = o; o = al256(o + bytes); return r; }
};
// main stream: high-priority queues, second stream: normal, bundle adjustment: lowest -- three pools, no sharing
// (orb_create_with_priority).  VIEO_TRACKER_PRIORITY=0: all normal (A/B).
inline int track_main_priority() {
  static const char* e = getenv("VIEO_TRACKER_PRIORITY");
  return e ? atoi(e) : 1;
}

// ---- the constants of a tracker's frames
struct TrackConstants {
  vieo_sbp_camera cam0;       // the constant part of a frame's search camera (Tcw_cur / Tcw_last: the prediction kernels)
  vieo_vio_frame f1_0, f2_0;  // ... and of its two optimiser problems
  float consts[32];           // inv_sigma2[16] | scale[16]
  vieo_camera pin_cam;        // the rectified pair's left camera for isInFrustum
  vieo_frustum_frame ff;      // (cams points at pin_cam or at the rig's cameras: a TrackConstants is built in place)
  float bounds[4][4];
};
// R: the rig as the tracker keeps it (null: a rectified pair), d_cams: its cameras in HBM
static void track_build_constants(TrackConstants& K, const vieo_tracker_params& P, const float* scale, const float* inv_sigma2,
                                  const vieo_tracker_rig* R, const vieo_camera* d_cams) {
  memset(&K, 0, sizeof(K));
  const vieo_camera* c0 = R ? &R->cams[0] : nullptr;
  const float fx = c0 ? c0->fx : P.fx, fy = c0 ? c0->fy : P.fy, cx = c0 ? c0->cx : P.cx, cy = c0 ? c0->cy : P.cy;
  vieo_sbp_camera& C = K.cam0;
  C.fx = fx, C.fy = fy, C.cx = cx, C.cy = cy;
  C.bounds[0] = 0, C.bounds[1] = (float)P.width, C.bounds[2] = 0, C.bounds[3] = (float)P.height;
  C.bf = P.bf, C.baseline = P.baseline, C.th = P.th_last, C.th_far = R ? R->th_far_pts : 0, C.mono = 0, C.nlevels = P.n_levels;
  for (int l = 0; l < P.n_levels; l++) C.scale[l] = scale[l], K.consts[l] = inv_sigma2[l], K.consts[16 + l] = scale[l];
  for (int c = 0; c < 4; c++) memcpy(K.bounds[c], C.bounds, 16);
  for (vieo_vio_frame* f : {&K.f1_0, &K.f2_0}) {
    memcpy(f->base.Rcb, P.Rcb, 72), memcpy(f->base.tcb, P.tcb, 24);
    f->base.fx = fx, f->base.fy = fy, f->base.cx = cx, f->base.cy = cy, f->base.bf = P.bf;
    if (R) f->base.n_cams = R->n_cams, f->base.cams = d_cams;
    memcpy(f->gw, P.gw, 24);
    f->inv_sigma_bg2 = P.inv_sigma_bg2, f->inv_sigma_ba2 = P.inv_sigma_ba2, f->th_depth = P.th_depth;
  }
  K.f2_0.compute_marg = 1;
  K.pin_cam.fx = P.fx, K.pin_cam.fy = P.fy, K.pin_cam.cx = P.cx, K.pin_cam.cy = P.cy;
  vieo_frustum_frame& F = K.ff;
  F.n_cams = 1, F.use_distort = 0, F.cams = &K.pin_cam, F.Tcr[0][0] = F.Tcr[0][5] = F.Tcr[0][10] = 1.f;
  memcpy(F.bounds, K.bounds, sizeof(F.bounds));
  F.bf = P.bf, F.n_levels = P.n_levels, F.viewing_cos_limit = 0.5f, F.log_scale_factor = logf(P.scale_factor);
  if (R) {
    F.n_cams = R->n_cams, F.use_distort = 1, F.cams = R->cams;
    for (int c = 0; c < R->n_cams; c++) {
      for (int r = 0; r < 3; r++) F.trc[c][r] = (float)R->Trc[c][r * 4 + 3];
      for (int i = 0; i < 12; i++) F.Tcr[c][i] = (float)R->Tcr[c][i];
    }
  }
}

// ---- a call's inputs: the fields both entries check (the images are the entry's own business), the capacities, and
// whether the local map a call names is the one in HBM (version / count of the table it would read)
inline bool track_input_ok(const vieo_track_input& I, int width) {
  return I.stride >= width && I.n_imu >= 0 && (I.n_imu == 0 || I.imu) && I.n_last >= 0 &&
         (I.n_last == 0 || (I.last_points && I.last_track_depth)) && I.n_local >= 0 && (I.n_local == 0 || I.local_alias);
}
inline bool track_input_fits(const vieo_track_input& I, int key_cap, int local_cap, int imu_cap) {
  return I.n_last <= key_cap && I.n_local <= local_cap && I.n_imu <= imu_cap;
}
inline bool track_local_changed(const vieo_track_input& I, int version_dev, int n_dev) {
  return I.n_local > 0 && (I.local_version != version_dev || I.n_local != n_dev);
}
// the per-call fields of an optimiser problem (the rest is TrackConstants' template)
inline void track_fill_problem(vieo_vio_frame& f, const vieo_track_input& I) {
  f.nav_last = I.nav_ref, f.dt_frames = I.t_cur - I.t_ref;
  f.last_has_prior = I.nav_prior && I.H_prior ? 1 : 0;
  if (f.last_has_prior) f.nav_prior = *I.nav_prior, memcpy(f.H_prior, I.H_prior, sizeof(f.H_prior));
  f.base.n_obs = 0, f.base.obs_begin = 0;
}
// an image plane into its pinned twin (nothing to do when the caller decoded it there)
inline void track_copy_plane(uint8_t* dst, const uint8_t* src, int width, int height, int stride) {
  if (src == dst) return;
  if (stride == width)
    memcpy(dst, src, (size_t)width * height);
  else
    for (int y = 0; y < height; y++) memcpy(dst + (size_t)y * width, src + (size_t)y * stride, width);
}
// Xw of n points (vieo_last_frame_point / vieo_frustum_point) as packed float[3]: the optimisers' point tables
template <class Point>
inline void track_pack_xyz(float* xyz, const Point* pts, int n) {
  for (int i = 0; i < n; i++) {
    const float* X = pts[i].Xw;
    xyz[3 * i] = X[0], xyz[3 * i + 1] = X[1], xyz[3 * i + 2] = X[2];
  }
}

// ---- what a frame's results decide
inline bool track_pre_ok(bool vision, int preint_status, double imu_dt) { return vision || (preint_status == 0 && imu_dt != 0); }
// Tracking.cc:311 (fewer than 10 matches with the IMU) / :1878 (fewer than 20 without): the reference returns before
// the optimisations; here they have run, their outputs are to be ignored
inline int track_status(bool vision, bool pre_ok, int n_matches_last) {
  return !pre_ok ? VIEO_TRACK_PREINT_FAILED : (n_matches_last < (vision ? 20 : 10) ? VIEO_TRACK_LOST : VIEO_TRACK_OK);
}
// Tracking.cc:301-309 / :1869-1876: the first search again with 2 x th
inline bool track_wants_wider_window(bool pre_ok, int n_matches_last) { return n_matches_last < 20 && pre_ok; }
// The layout-free fields of a frame's output (*o is cleared first; the key tables are the caller's).  imu: null = none;
// r1 / r2: result_bytes of a vieo_vio_result (vision only: its leading vieo_pose_result, the rest stays zero).
inline void track_fill_output(vieo_track_output* o, bool vision, int preint_status, int nm_last, int nm_local, int widened,
                              const vieo_navstate& nav_pred,
                              const vieo_imu_preint* imu, const void* r1, const void* r2, size_t result_bytes, float ms_gpu,
                              float ms_host) {
  memset(o, 0, sizeof(*o));
  o->preint_status = preint_status;
  o->status = track_status(vision, track_pre_ok(vision, preint_status, imu ? imu->dt : 0.0), nm_last);
  o->n_matches_last = nm_last, o->n_matches_local = nm_local, o->widened = widened, o->nav_pred = nav_pred;
  if (imu) o->imu = *imu;
  memcpy(&o->first, r1, result_bytes), memcpy(&o->second, r2, result_bytes);
  o->ms_gpu = ms_gpu, o->ms_host = ms_host;
}

// ---- the chain behind the prediction.  The arrays of a call's n frames as its launches read them: [n][capacity] each.
struct TrackChain {
  int n, kc, pcap, n_cams;  // frames; keys and points (keys + local candidates) per frame; cameras the searches loop over
  bool rig, vision;
  hipStream_t st;
  // the frames: mvKeys / mDescriptors, uright, the image bounds, the key counts ({n, -} per frame: the left image's / a
  // rig's {N, 0}), a rig's first key per camera
  const vieo_keypoint* kp;
  const uint8_t* desc;
  const float *uright, *bounds;
  const int32_t *cnt, *cam_first;
  // the searches' queries (first: a rig's are compacted; second: the owner's step writes them), counts, capacities; rigs:
  // the last frame's points and the (key, camera) pair behind every compacted query
  const vieo_proj_query* q1;
  vieo_proj_query* q2;
  const int32_t *nq1, *query_src;
  const vieo_last_frame_point* same_point;
  int q1_cap, q2_cap;
  int32_t *nq2, *assign, *mpref, *obskey;
  uint8_t *taken, *held, *outl, *key_outlier;  // (outl: per observation, key_outlier: per key, k_track_finish)
  vieo_pose_obs* obs;
  float *xyz, *dep;     // point tables [n][pcap]: last frame's points | local candidates
  const float* consts;  // inv_sigma2[16] | scale[16]
  // the two optimisations' problems and results: vieo_vio_* or, vision only, vieo_pose_* records
  void *f1, *f2, *r1, *r2;
  size_t fstride;
  int32_t *nm1, *nm2, *nobs2;  // matches of the two searches, observations of the second optimisation
  float nn_last, nn_local, close;
};

// project(): the first search's queries from the predicted pose, skipped when `projected` (made beside the extraction).
// before_local_map(): behind the first optimisation's launch, where the host gets ahead of the device again.
// local_queries(): isInFrustum of the local map's candidates into c.q2 / c.nq2 and c.dep + kc.
template <class Project, class BeforeLocalMap, class LocalQueries>
static int track_run_chain(const TrackChain& c, bool projected, Project&& project, BeforeLocalMap&& before_local_map,
                           LocalQueries&& local_queries) {
  const int n = c.n, kc = c.kc, nc = c.n_cams, vio = c.vision ? 0 : 1;
  hipStream_t st = c.st;
  const auto search = [&](int mode, const vieo_proj_query* q, const int32_t* d_nq, int q_cap, const uint8_t* taken, float nn,
                          int32_t* d_nm) {
    if (c.rig)
      return vieo_search_by_projection_rig_batch_device(mode, q, d_nq, q_cap, n, c.kp, c.uright, c.desc, taken, c.cam_first, kc,
                                                        c.bounds, nc, nn, 1, c.assign, d_nm, st);
    return vieo_search_by_projection_batch_device(mode, q, d_nq, q_cap, n, c.kp, c.uright, c.desc, taken, c.cnt, kc, 0, 2, c.bounds,
                                                  nn, 1, c.assign, d_nm, st);
  };
  // the search's assignment merged into the frames' point tables and the observations gathered from it: one launch
  const auto merge_build_obs = [&](void* frames, int point_offset, int reset, const vieo_last_frame_point* same_point,
                                   const int32_t* query_src, int q_cap) {
    return vieo_track_merge_build_obs_batch_device(c.assign, c.mpref, point_offset, reset, nc, same_point, query_src, q_cap, c.xyz,
                                                   c.vision ? nullptr : c.dep, c.close, c.pcap, c.kp, c.uright, c.cnt,
                                                   c.rig ? c.cam_first : nullptr, nc, kc, n, 0, c.rig ? 1 : 2, c.consts, c.obs,
                                                   c.obskey, frames, vio, st);
  };
  const auto pose = [&](void* frames, void* results) {
    if (c.vision)
      return vieo_pose_optimization_batch_device_ex((const vieo_pose_frame*)frames, n, c.obs, c.outl, (vieo_pose_result*)results,
                                                    VIEO_POSE_CAMS_RECTIFIED, st);
    return vieo_pose_optimization_vio_batch_device_ex((const vieo_vio_frame*)frames, n, c.obs, c.outl, (vieo_vio_result*)results,
                                                      c.rig ? VIEO_POSE_CAMS_RIG : VIEO_POSE_CAMS_RECTIFIED, VIEO_POSE_ENC_NONE, st);
  };
  int rc;
  if (!projected && (rc = project()) != VIEO_OK) return rc;
  if ((rc = search(VIEO_SBP_LAST_FRAME, c.q1, c.nq1, c.q1_cap, nullptr, c.nn_last, c.nm1)) != VIEO_OK) return rc;
  if ((rc = merge_build_obs(c.f1, 0, 1, c.same_point, c.query_src, c.same_point ? c.q1_cap : 0)) != VIEO_OK) return rc;
  if ((rc = pose(c.f1, c.r1)) != VIEO_OK) return rc;
  if ((rc = before_local_map()) != VIEO_OK) return rc;
  rc = vieo_track_after_pose_held_batch_device(c.mpref, c.obskey, c.outl, c.f1, c.r1, vio, kc, n, c.f2, c.taken, c.cnt, 0, 2,
                                               c.held, c.pcap, st);
  if (rc != VIEO_OK) return rc;
  if ((rc = local_queries()) != VIEO_OK) return rc;
  (void)vieo_sbp_keep_grid(1);  // the frames' keys have not changed since the first search
  if ((rc = search(VIEO_SBP_LOCAL_MAP, c.q2, c.nq2, c.q2_cap, c.taken, c.nn_local, c.nm2)) != VIEO_OK) return rc;
  if ((rc = merge_build_obs(c.f2, kc, 0, nullptr, nullptr, 0)) != VIEO_OK) return rc;
  if ((rc = pose(c.f2, c.r2)) != VIEO_OK) return rc;
  hipLaunchKernelGGL(k_track_finish, dim3(n), dim3(256), 0, st, c.obskey, c.outl, (const uint8_t*)c.f2, c.fstride, c.key_outlier,
                     kc, c.nobs2);
  VIEO_HIP_CHECK(hipGetLastError());
  return VIEO_OK;
}

}  // namespace vieo
