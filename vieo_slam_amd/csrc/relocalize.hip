// relocalize.hip -- bool Tracking::Relocalization() (reference src/Tracking.cc:2541-2663) for one lost frame, of the
// rectified configuration (vieo_relocalize) or of a 1- to 4-camera rig with Frame::usedistort_ (vieo_relocalize_rig),
// on the host around the library's own entries; one implementation (reloc_run) takes the form named after the slash
// for a rig frame:
//   vieo_search_by_bow / _rig     SearchByBoW of every candidate, one call            (:2556-2574)
//   vieo_pnp_create / _rig        every RANSAC hypothesis of every kept candidate, Refine per record, one call
//   vieo_pnp_iterate              the round-robin while over the candidates, 5 iterations a visit  (:2581-2598)
//   vieo_pose_optimization        PoseOptimization, from the frame's float Tcw and back to it   (:2617,2631,2646); rig:
//                                 n_cams / cams, the key's camera in bits 8..11 of the observation's flags
//   vieo_sbp_project_keyframe(rig) + vieo_search_by_projection / _rig (VIEO_SBP_RELOC)   the two widening searches
//                                 (:2628,2642)
// The decisions between the stages are sequential in the reference and stay here.  The frame's state is what the
// reference keeps in mCurrentFrame: Tcw (float), mvpMapPoints as the candidate's key per frame key, mvbOutlier (written
// by an optimisation only for keys that hold a point then).
#include <algorithm>
#include <cmath>
#include <unordered_set>
#include <vector>

#include "common.h"

namespace vieo {

// Frame::UpdateNavStatePVRFromTcw: Twb = (Tbc * Tcw)^-1 in double from the float Tcw
static void reloc_nav_from_tcw(const float* Tcw, const double* Rcb, const double* tcb, vieo_navstate& nav) {
  double Rbw[9], tbw[3], tbc[3];
  for (int i = 0; i < 3; i++) tbc[i] = -((Rcb[i] * tcb[0] + Rcb[3 + i] * tcb[1]) + Rcb[6 + i] * tcb[2]);
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++)
      Rbw[i * 3 + j] = (Rcb[i] * (double)Tcw[j] + Rcb[3 + i] * (double)Tcw[4 + j]) + Rcb[6 + i] * (double)Tcw[8 + j];
    tbw[i] = ((Rcb[i] * (double)Tcw[3] + Rcb[3 + i] * (double)Tcw[7]) + Rcb[6 + i] * (double)Tcw[11]) + tbc[i];
  }
  double R[9];  // Rwb
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R[i * 3 + j] = Rbw[j * 3 + i];
  for (int i = 0; i < 3; i++) nav.p[i] = -((R[i * 3] * tbw[0] + R[i * 3 + 1] * tbw[1]) + R[i * 3 + 2] * tbw[2]);
  // unit quaternion (w, x, y, z) of Rwb, largest component first
  const double tr = R[0] + R[4] + R[8];
  double q[4];
  if (tr > 0) {
    const double s = std::sqrt(tr + 1.0) * 2;
    q[0] = 0.25 * s, q[1] = (R[7] - R[5]) / s, q[2] = (R[2] - R[6]) / s, q[3] = (R[3] - R[1]) / s;
  } else if (R[0] > R[4] && R[0] > R[8]) {
    const double s = std::sqrt(1.0 + R[0] - R[4] - R[8]) * 2;
    q[0] = (R[7] - R[5]) / s, q[1] = 0.25 * s, q[2] = (R[1] + R[3]) / s, q[3] = (R[2] + R[6]) / s;
  } else if (R[4] > R[8]) {
    const double s = std::sqrt(1.0 + R[4] - R[0] - R[8]) * 2;
    q[0] = (R[2] - R[6]) / s, q[1] = (R[1] + R[3]) / s, q[2] = 0.25 * s, q[3] = (R[5] + R[7]) / s;
  } else {
    const double s = std::sqrt(1.0 + R[8] - R[0] - R[4]) * 2;
    q[0] = (R[3] - R[1]) / s, q[1] = (R[2] + R[6]) / s, q[2] = (R[5] + R[7]) / s, q[3] = 0.25 * s;
  }
  const double n = std::sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
  for (int i = 0; i < 4; i++) nav.q[i] = q[i] / n;
}

// Frame::UpdatePoseFromNS: Rcw = (Rwb * Rbc)^T, tcw = -Rcw * (Rwb * tbc + pwb), rounded to float
static void reloc_tcw_from_nav(const vieo_navstate& nav, const double* Rcb, const double* tcb, float* Tcw) {
  const double w = nav.q[0], x = nav.q[1], y = nav.q[2], z = nav.q[3];
  const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                       2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                       2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
  double tbc[3], pwc[3];
  for (int i = 0; i < 3; i++) tbc[i] = -((Rcb[i] * tcb[0] + Rcb[3 + i] * tcb[1]) + Rcb[6 + i] * tcb[2]);
  for (int i = 0; i < 3; i++) pwc[i] = ((R[i * 3] * tbc[0] + R[i * 3 + 1] * tbc[1]) + R[i * 3 + 2] * tbc[2]) + nav.p[i];
  for (int i = 0; i < 3; i++) {
    double row[3];  // row i of Rcw = Rcb * Rwb^T
    for (int j = 0; j < 3; j++) row[j] = (Rcb[i * 3] * R[j * 3] + Rcb[i * 3 + 1] * R[j * 3 + 1]) + Rcb[i * 3 + 2] * R[j * 3 + 2];
    for (int j = 0; j < 3; j++) Tcw[i * 4 + j] = (float)row[j];
    Tcw[i * 4 + 3] = (float)(-((row[0] * pwc[0] + row[1] * pwc[1]) + row[2] * pwc[2]));
  }
  Tcw[12] = Tcw[13] = Tcw[14] = 0.f, Tcw[15] = 1.f;
}

static bool reloc_frame_ok(const vieo_reloc_frame& F) {
  if (F.n_keys < 0 || F.n_levels < 1 || F.n_levels > 16 || F.n_nodes < 0) return false;
  if (!F.level_sigma2 || !F.inv_level_sigma2 || !F.scale_factor) return false;
  if (F.n_keys > 0 && (!F.keys || !F.uright || !F.descriptors)) return false;
  for (int i = 0; i < F.n_keys; i++)
    if (F.keys[i].octave < 0 || F.keys[i].octave >= F.n_levels) return false;
  return true;
}

// the rig of vieo_relocalize_rig against its frame: 1..4 cameras, the same number everywhere, cam_first a partition of
// the frame's keys in camera-major order
static bool reloc_rig_ok(const vieo_reloc_frame& F, const vieo_reloc_rig& R) {
  const int nc = R.pnp.n_cams;
  if (nc < 1 || nc > 4 || F.n_cams != nc || !R.cam_first || !R.sbp || !R.pose_cams || R.sbp->n_cams != nc) return false;
  if (R.cam_first[0] != 0 || R.cam_first[nc] != F.n_keys) return false;
  for (int c = 0; c < nc; c++)
    if (R.cam_first[c + 1] < R.cam_first[c]) return false;
  return true;
}

// Both entries.  rig == nullptr: the rectified configuration (vieo_relocalize); otherwise the frame of a camera rig
// (vieo_relocalize_rig), whose four stages take their rig forms -- the decisions between them are the same.
static int reloc_run(const vieo_reloc_frame* frame, const vieo_reloc_rig* rig, const vieo_reloc_candidate* cands,
                     int n_cands, const int32_t* samples, int n_rows, uint64_t seed, vieo_reloc_result* result,
                     int32_t* mp_ref, uint8_t* outlier, vieo_reloc_visit* trace, int32_t trace_capacity) {
  if (!frame || !cands || n_cands <= 0 || !result || trace_capacity < 0 || (trace_capacity > 0 && !trace)) return VIEO_E_INVALID;
  const vieo_reloc_frame& F = *frame;
  if (!rig && F.n_cams != 0) {
    set_error("Relocalization: a rig frame (n_cams = %d) goes to vieo_relocalize_rig", F.n_cams);
    return VIEO_E_INVALID;
  }
  if (rig && (F.n_keys < 0 || !reloc_rig_ok(F, *rig))) {
    set_error("Relocalization: the rig is inconsistent (1..4 cameras in frame, pnp and sbp; cam_first from 0 to n_keys, not decreasing)");
    return VIEO_E_INVALID;
  }
  const int n_cams = rig ? rig->pnp.n_cams : 0;
  if (n_rows <= 0 || n_rows > 512) {
    set_error("Relocalization: %d sample rows, 1..512", n_rows);
    return VIEO_E_INVALID;
  }
  if (!reloc_frame_ok(F) || (F.n_keys > 0 && (!mp_ref || !outlier))) {
    set_error("Relocalization: the frame is inconsistent (pointers, 1..16 levels, octaves in range)");
    return VIEO_E_INVALID;
  }
  for (int c = 0; c < n_cands; c++)
    if (cands[c].kf.n_keys < 0 || (cands[c].kf.n_keys > 0 && (!cands[c].points || !cands[c].kf.mp_id))) {
      set_error("Relocalization: candidate %d is inconsistent", c);
      return VIEO_E_INVALID;
    }
  const int N = F.n_keys;
  int n_visits = 0;
  auto visit = [&](const vieo_reloc_visit& v) {
    if (n_visits < trace_capacity) trace[n_visits] = v;
    n_visits++;
  };
  const vieo_reloc_visit blank{-1, 0, -1, 0, 0, 0, {-1, -1, -1}, {-1, -1}, 0};
  // ---- SearchByBoW of every candidate, ORBmatcher(0.75, true); fewer than 15 matches: discarded
  vieo_bow_keys fk;
  fk.n_keys = N, fk.n_nodes = F.n_nodes, fk.keys = F.keys, fk.descriptors = F.descriptors, fk.mp_id = nullptr;
  fk.node_id = F.node_id, fk.node_first = F.node_first, fk.node_feat = F.node_feat;
  std::vector<vieo_bow_keys> kfs(n_cands);
  for (int c = 0; c < n_cands; c++) kfs[c] = cands[c].kf;
  std::vector<int32_t> match((size_t)n_cands * std::max(N, 1)), n_matches(n_cands);
  std::vector<uint8_t> key_cam;  // get<0>(mapn2in_[j]) of a rig frame
  if (rig) {
    key_cam.assign(std::max(N, 1), 0);
    for (int c = 0; c < n_cams; c++) std::fill(key_cam.begin() + rig->cam_first[c], key_cam.begin() + rig->cam_first[c + 1], (uint8_t)c);
  }
  int rc = rig ? vieo_search_by_bow_rig(&fk, key_cam.data(), n_cams, kfs.data(), n_cands, 0.75f, 1, match.data(), n_matches.data())
               : vieo_search_by_bow(&fk, kfs.data(), n_cands, 0.75f, 1, match.data(), n_matches.data());
  if (rc != VIEO_OK) return rc;
  std::vector<uint8_t> discarded(n_cands, 0);
  std::vector<int> solver_of(n_cands, -1), calls(n_cands, 0);
  // ---- PnPsolver of the kept candidates (the constructor's vectors), SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991)
  struct Corr {
    std::vector<float> Xw, uv, s2;
    std::vector<int32_t> key;
    std::vector<uint8_t> cam;  // mapidx2cami_ (rig)
  };
  std::vector<Corr> corr;
  std::vector<vieo_pnp_candidate> pc;
  std::vector<int32_t> smp;
  int nCandidates = 0;
  for (int c = 0; c < n_cands; c++) {
    vieo_reloc_visit v = blank;
    v.cand = c, v.n_inliers = n_matches[c];
    if (n_matches[c] < 15) {
      discarded[c] = 1, v.no_more = 1;
      visit(v);
      continue;
    }
    visit(v);
    solver_of[c] = nCandidates++;
    corr.emplace_back();
    Corr& Q = corr.back();
    const int32_t* m = &match[(size_t)c * N];
    for (int j = 0; j < N; j++) {
      if (m[j] < 0) continue;
      const vieo_keyframe_point& P = cands[c].points[m[j]];
      Q.Xw.insert(Q.Xw.end(), P.Xw, P.Xw + 3);
      Q.uv.push_back(F.keys[j].x), Q.uv.push_back(F.keys[j].y);
      Q.s2.push_back(F.level_sigma2[F.keys[j].octave]);
      Q.key.push_back(j);
      if (rig) Q.cam.push_back(key_cam[j]);
    }
    if (samples) smp.insert(smp.end(), samples + (size_t)c * n_rows * 4, samples + (size_t)(c + 1) * n_rows * 4);
  }
  memset(result, 0, sizeof(*result));
  result->cand = -1;
  std::fill(mp_ref, mp_ref + N, -1);
  std::fill(outlier, outlier + N, (uint8_t)0);
  result->n_visits = n_visits;
  if (nCandidates == 0) return VIEO_OK;
  for (Corr& Q : corr)
    pc.push_back(vieo_pnp_candidate{(int32_t)Q.key.size(), N, Q.Xw.data(), Q.uv.data(), Q.s2.data(), Q.key.data(), F.fx, F.fy,
                                    F.cx, F.cy});
  const vieo_pnp_params par{0.99, 10, 300, 4, 0.5f, 5.991f, 0};
  vieo_pnp* pnp = nullptr;
  if (rig) {
    std::vector<const uint8_t*> cam_of;
    for (Corr& Q : corr) cam_of.push_back(Q.cam.data());
    rc = vieo_pnp_create_rig(&pnp, pc.data(), nCandidates, cam_of.data(), &rig->pnp, &par, samples ? smp.data() : nullptr, n_rows, seed);
  } else
    rc = vieo_pnp_create(&pnp, pc.data(), nCandidates, &par, samples ? smp.data() : nullptr, n_rows, seed);
  if (rc != VIEO_OK) return rc;
  // ---- the frame's state and the stages
  float Tcw[16];
  std::vector<uint8_t> inl(std::max(N, 1)), taken(std::max(N, 1)), outl;
  std::vector<int32_t> assign(std::max(N, 1)), obs_key;
  std::vector<vieo_pose_obs> obs;
  std::vector<vieo_keyframe_point> pts;
  std::vector<vieo_proj_query> queries;
  vieo_navstate nav;
  memset(&nav, 0, sizeof(nav));
  auto optimise = [&](int c, int* nGood) -> int {  // Optimizer::PoseOptimization(&mCurrentFrame)
    obs.clear(), obs_key.clear();
    for (int j = 0; j < N; j++) {
      if (mp_ref[j] < 0) continue;
      const vieo_keyframe_point& P = cands[c].points[mp_ref[j]];
      obs.push_back(vieo_pose_obs{{P.Xw[0], P.Xw[1], P.Xw[2]}, F.keys[j].x, F.keys[j].y, F.uright[j],
                                  F.inv_level_sigma2[F.keys[j].octave], rig ? (int32_t)key_cam[j] << 8 : 0});
      obs_key.push_back(j);
    }
    vieo_pose_frame pf;
    memset(&pf, 0, sizeof(pf));
    reloc_nav_from_tcw(Tcw, F.Rcb, F.tcb, nav);
    pf.nav = nav;
    memcpy(pf.Rcb, F.Rcb, sizeof(pf.Rcb)), memcpy(pf.tcb, F.tcb, sizeof(pf.tcb));
    pf.fx = F.fx, pf.fy = F.fy, pf.cx = F.cx, pf.cy = F.cy, pf.bf = F.bf, pf.n_obs = (int32_t)obs.size();
    if (rig) pf.n_cams = n_cams, pf.cams = rig->pose_cams;
    outl.assign(std::max<size_t>(obs.size(), 1), 0);
    vieo_pose_result res;
    memset(&res, 0, sizeof(res));
    const int r = vieo_pose_optimization(&pf, obs.data(), outl.data(), &res);
    if (r != VIEO_OK) return r;
    *nGood = res.n_inliers;
    if (res.status != VIEO_POSE_OK) return VIEO_OK;  // fewer than 3 correspondences: returns 0, nothing written
    for (size_t k = 0; k < obs_key.size(); k++) outlier[obs_key[k]] = outl[k];
    nav = res.nav;
    reloc_tcw_from_nav(nav, F.Rcb, F.tcb, Tcw);
    return VIEO_OK;
  };
  auto erase_outliers = [&]() {
    for (int j = 0; j < N; j++)
      if (outlier[j]) mp_ref[j] = -1;
  };
  // matcher2.SearchByProjection(mCurrentFrame, pKF, sFound, th, ORBdist)
  auto search = [&](int c, const std::unordered_set<int32_t>& sFound, float th, float orb_dist, int* nadditional) -> int {
    const vieo_reloc_candidate& C = cands[c];
    pts.assign(C.points, C.points + C.kf.n_keys);
    for (int k = 0; k < C.kf.n_keys; k++)
      if (C.kf.mp_id[k] < 0 || sFound.count(C.kf.mp_id[k])) pts[k].flags &= ~1;
    vieo_sbp_camera cam;
    memset(&cam, 0, sizeof(cam));
    for (int i = 0; i < 12; i++) cam.Tcw_cur[i] = cam.Tcw_last[i] = (double)Tcw[i];
    cam.fx = F.fx, cam.fy = F.fy, cam.cx = F.cx, cam.cy = F.cy, cam.bf = F.bf, cam.baseline = F.bf / F.fx;
    memcpy(cam.bounds, F.bounds, sizeof(cam.bounds));
    cam.th = th, cam.th_far = 0, cam.mono = 0, cam.nlevels = F.n_levels;
    for (int l = 0; l < F.n_levels; l++) cam.scale[l] = F.scale_factor[l];
    const int per_point = rig ? n_cams : 1;  // a query per (map point, camera), point-major
    queries.resize(std::max(C.kf.n_keys * per_point, 1));
    int r = vieo_sbp_project_keyframe(pts.data(), C.kf.n_keys, &cam, rig ? rig->sbp : nullptr, F.log_scale_factor, queries.data());
    if (r != VIEO_OK) return r;
    for (int j = 0; j < N; j++) taken[j] = mp_ref[j] >= 0;
    int32_t nm = 0;
    if (rig)
      r = vieo_search_by_projection_rig(VIEO_SBP_RELOC, queries.data(), C.kf.n_keys * per_point, F.keys, F.uright, F.descriptors,
                                        taken.data(), N, rig->cam_first, &rig->sbp->bounds[0][0], n_cams, orb_dist, 1,
                                        assign.data(), &nm);
    else
      r = vieo_search_by_projection(VIEO_SBP_RELOC, queries.data(), C.kf.n_keys, F.keys, F.uright, F.descriptors, taken.data(),
                                    N, F.bounds, orb_dist, 1, assign.data(), &nm);
    if (r != VIEO_OK) return r;
    for (int j = 0; j < N; j++) {
      if (assign[j] >= 0) mp_ref[j] = assign[j] / per_point;
      else if (assign[j] == VIEO_SBP_ERASED) mp_ref[j] = -1;
    }
    *nadditional = nm;
    return VIEO_OK;
  };
  bool bMatch = false;
  rc = VIEO_OK;
  while (nCandidates > 0 && !bMatch && rc == VIEO_OK) {
    for (int c = 0; c < n_cands && rc == VIEO_OK; c++) {
      if (discarded[c]) continue;
      vieo_reloc_visit v = blank;
      v.cand = c, v.call = ++calls[c];
      int32_t found = 0, nInliers = 0, bNoMore = 0, row = -1;
      rc = vieo_pnp_iterate(pnp, solver_of[c], 5, &found, Tcw, inl.data(), &nInliers, &bNoMore, &row);
      if (rc == VIEO_E_CAPACITY) rc = VIEO_OK, found = 0, bNoMore = 2;  // the sample table is used up: no more draws
      if (rc != VIEO_OK) break;
      v.row = row, v.no_more = bNoMore, v.found = found, v.n_inliers = nInliers;
      if (bNoMore) discarded[c] = 1, nCandidates--;
      if (!found) {
        visit(v);
        continue;
      }
      const int32_t* m = &match[(size_t)c * N];
      std::unordered_set<int32_t> sFound;
      for (int j = 0; j < N; j++) {
        mp_ref[j] = inl[j] ? m[j] : -1;
        if (inl[j]) sFound.insert(cands[c].kf.mp_id[m[j]]);
      }
      int nGood = 0;
      if ((rc = optimise(c, &nGood)) != VIEO_OK) break;
      v.n_good[0] = nGood;
      if (nGood < 10) {
        visit(v);
        continue;
      }
      erase_outliers();
      if (nGood < 50) {
        int nadditional = 0;
        if ((rc = search(c, sFound, 10.f, 100.f, &nadditional)) != VIEO_OK) break;
        v.n_additional[0] = nadditional;
        if (nadditional + nGood >= 50) {
          if ((rc = optimise(c, &nGood)) != VIEO_OK) break;
          v.n_good[1] = nGood;
          if (nGood > 30 && nGood < 50) {
            sFound.clear();
            for (int j = 0; j < N; j++)
              if (mp_ref[j] >= 0) sFound.insert(cands[c].kf.mp_id[mp_ref[j]]);
            if ((rc = search(c, sFound, 3.f, 64.f, &nadditional)) != VIEO_OK) break;
            v.n_additional[1] = nadditional;
            if (nGood + nadditional >= 50) {
              if ((rc = optimise(c, &nGood)) != VIEO_OK) break;
              v.n_good[2] = nGood;
              erase_outliers();
            }
          }
        }
      }
      visit(v);
      if (nGood >= 50) {
        bMatch = true;
        result->found = 1, result->cand = c, result->n_good = nGood;
        break;
      }
    }
  }
  vieo_pnp_destroy(pnp);
  if (rc != VIEO_OK) return rc;
  result->n_visits = n_visits;
  if (bMatch) {
    result->nav = nav;
    memcpy(result->Tcw, Tcw, sizeof(Tcw));
  } else {
    std::fill(mp_ref, mp_ref + N, -1);
    std::fill(outlier, outlier + N, (uint8_t)0);
  }
  if (n_visits > trace_capacity) {
    set_error("Relocalization: %d visits, the trace holds %d", n_visits, trace_capacity);
    return VIEO_E_CAPACITY;
  }
  return VIEO_OK;
}

}  // namespace vieo

extern "C" int vieo_relocalize(const vieo_reloc_frame* frame, const vieo_reloc_candidate* cands, int n_cands,
                               const int32_t* samples, int n_rows, uint64_t seed, vieo_reloc_result* result,
                               int32_t* mp_ref, uint8_t* outlier, vieo_reloc_visit* trace, int32_t trace_capacity) {
  return vieo::reloc_run(frame, nullptr, cands, n_cands, samples, n_rows, seed, result, mp_ref, outlier, trace, trace_capacity);
}

extern "C" int vieo_relocalize_rig(const vieo_reloc_frame* frame, const vieo_reloc_rig* rig, const vieo_reloc_candidate* cands,
                                   int n_cands, const int32_t* samples, int n_rows, uint64_t seed, vieo_reloc_result* result,
                                   int32_t* mp_ref, uint8_t* outlier, vieo_reloc_visit* trace, int32_t trace_capacity) {
  if (!rig) return VIEO_E_INVALID;
  return vieo::reloc_run(frame, rig, cands, n_cands, samples, n_rows, seed, result, mp_ref, outlier, trace, trace_capacity);
}
