// loop_compute_sim3.hip -- bool LoopClosing::ComputeSim3() (reference src/LoopClosing.cc:308-444) up to bMatch, on the
// host around the library's own entries:
//   vieo_search_by_bow_kf      SearchByBoW of every candidate, one call                       (:341-350)
//   vieo_sim3_create           every RANSAC hypothesis of every kept candidate, one call      (:353-357)
//   vieo_sim3_iterate          the round-robin while over the candidates, 5 iterations a visit (:380)
//   vieo_search_by_sim3        all visits of a pass that returned a Sim3, one call             (:404)
//   vieo_optimize_sim3         the same visits, one launch                                     (:411)
// The decisions between the stages are sequential in the reference and stay here.
#include <algorithm>
#include <vector>

#include "common.h"

namespace vieo {

// what the Sim3Solver constructor and the entries below index without a check of their own
static bool loop_kf_ok(const vieo_loop_keyframe& K) {
  const int n = K.bow.n_keys;
  if (n < 0 || K.n_levels < 1 || K.n_levels > 16 || K.n_cams < 1 || K.n_cams > 4 || !K.cams) return false;
  if (n > 0 && (!K.bow.keys || !K.bow.descriptors || !K.bow.mp_id || !K.points)) return false;
  for (int i = 0; i < n; i++) {
    const int c = K.cam_of_key ? K.cam_of_key[i] : 0, o = K.bow.keys[i].octave;
    if (c < 0 || c >= K.n_cams || o < 0 || o >= K.n_levels) return false;
  }
  return true;
}

// Sim3Solver's camera table of one key frame: the rig with GetTcr() in Rcb / tcb, or one pinhole with the identity
static void sim3_cameras(const vieo_loop_keyframe& K, std::vector<vieo_camera>& out) {
  out.clear();
  if (!K.use_distort) {
    vieo_camera c;
    memset(&c, 0, sizeof(c));
    c.model = VIEO_CAM_PINHOLE;
    c.fx = K.cams[0].fx, c.fy = K.cams[0].fy, c.cx = K.cams[0].cx, c.cy = K.cams[0].cy;
    c.Rcb[0] = c.Rcb[4] = c.Rcb[8] = 1.0;
    out.push_back(c);
    return;
  }
  for (int i = 0; i < K.n_cams; i++) {
    vieo_camera c = K.cams[i];
    for (int r = 0; r < 3; r++) {
      for (int k = 0; k < 3; k++) c.Rcb[r * 3 + k] = (double)K.Tcr[i][r * 4 + k];
      c.tcb[r] = (double)K.Tcr[i][r * 4 + 3];
    }
    out.push_back(c);
  }
}

static inline void cam_point(const vieo_loop_keyframe& K, const float* Xw, float* X) {
  for (int r = 0; r < 3; r++) X[r] = ((K.Rcw[r * 3] * Xw[0] + K.Rcw[r * 3 + 1] * Xw[1]) + K.Rcw[r * 3 + 2] * Xw[2]) + K.tcw[r];
}

}  // namespace vieo

extern "C" int vieo_compute_sim3(const vieo_loop_keyframe* kf1, const vieo_loop_keyframe* cands, int n_cands, int thresh_matches,
                                 int min_inliers, int fix_scale, const int32_t* samples, int n_rows, uint64_t seed,
                                 vieo_compute_sim3_result* result, int32_t* match12, vieo_compute_sim3_visit* trace,
                                 int32_t trace_capacity) {
  using namespace vieo;
  if (!kf1 || !cands || n_cands <= 0 || !result || trace_capacity < 0 || (trace_capacity > 0 && !trace) || n_rows <= 0 ||
      n_rows > 512 || min_inliers < 3) {
    set_error("ComputeSim3: a null pointer, no candidate, %d sample rows (1..512) or min_inliers = %d (>= 3)", n_rows, min_inliers);
    return VIEO_E_INVALID;
  }
  if (!loop_kf_ok(*kf1) || (kf1->bow.n_keys > 0 && !match12)) {
    set_error("ComputeSim3: the current key frame is inconsistent (pointers, 1..16 levels, 1..4 cameras, octaves and cameras in range)");
    return VIEO_E_INVALID;
  }
  for (int c = 0; c < n_cands; c++)
    if (!loop_kf_ok(cands[c])) {
      set_error("ComputeSim3: candidate %d is inconsistent (pointers, 1..16 levels, 1..4 cameras, octaves and cameras in range)", c);
      return VIEO_E_INVALID;
    }
  const int N1 = kf1->bow.n_keys;
  int n_visits = 0;
  auto visit = [&](const vieo_compute_sim3_visit& v) {
    if (n_visits < trace_capacity) trace[n_visits] = v;
    n_visits++;
  };
  const vieo_compute_sim3_visit blank{-1, 0, -1, 0, 0, 0, -1, -1};
  // ---- 1. SearchByBoW of every candidate, ORBmatcher(0.75, true)
  std::vector<vieo_bow_keys> bows(n_cands);
  for (int c = 0; c < n_cands; c++) bows[c] = cands[c].bow;
  std::vector<int32_t> match((size_t)n_cands * std::max(N1, 1)), n_matches(n_cands);
  int rc = vieo_search_by_bow_kf(&kf1->bow, bows.data(), n_cands, 0.75f, 1, match.data(), n_matches.data());
  if (rc != VIEO_OK) return rc;
  // ---- 2. the Sim3Solver constructor of the kept candidates
  struct Corr {
    std::vector<float> X1, X2;
    std::vector<int32_t> e1, e2, i1, c1, c2;
    std::vector<vieo_camera> cams2;
  };
  std::vector<uint8_t> discarded(n_cands, 0);
  std::vector<int> solver_of(n_cands, -1), calls(n_cands, 0);
  std::vector<Corr> corr;
  corr.reserve(n_cands);
  std::vector<vieo_camera> cams1;
  sim3_cameras(*kf1, cams1);
  std::vector<int32_t> smp;
  std::vector<std::pair<int, int>> by_id;  // (mp_id, key) of the candidate, ascending: GetIndexInKeyFrame
  int nCandidates = 0;
  for (int c = 0; c < n_cands; c++) {
    vieo_compute_sim3_visit v = blank;
    v.cand = c, v.n_inliers = n_matches[c];
    if (n_matches[c] < thresh_matches) {
      discarded[c] = 1, v.no_more = 1;
      visit(v);
      continue;
    }
    visit(v);
    solver_of[c] = nCandidates++;
    corr.emplace_back();
    Corr& Q = corr.back();
    const vieo_loop_keyframe& K2 = cands[c];
    sim3_cameras(K2, Q.cams2);
    by_id.clear();
    for (int k = 0; k < K2.bow.n_keys; k++)
      if (K2.bow.mp_id[k] >= 0) by_id.emplace_back(K2.bow.mp_id[k], k);
    std::sort(by_id.begin(), by_id.end());
    const int32_t* m = &match[(size_t)c * N1];
    for (int i1 = 0; i1 < N1; i1++) {
      if (m[i1] < 0 || K2.bow.mp_id[m[i1]] < 0 || kf1->bow.mp_id[i1] < 0) continue;
      const int id2 = K2.bow.mp_id[m[i1]];
      float X1[3], X2[3];
      cam_point(*kf1, kf1->points[i1].Xw, X1);
      cam_point(K2, K2.points[m[i1]].Xw, X2);
      for (auto it = std::lower_bound(by_id.begin(), by_id.end(), std::make_pair(id2, -1)); it != by_id.end() && it->first == id2; ++it) {
        const int i2 = it->second;
        Q.e1.push_back((int32_t)(size_t)(9.210 * (double)kf1->level_sigma2[kf1->bow.keys[i1].octave]));
        Q.e2.push_back((int32_t)(size_t)(9.210 * (double)K2.level_sigma2[K2.bow.keys[i2].octave]));
        Q.i1.push_back(i1);
        Q.X1.insert(Q.X1.end(), X1, X1 + 3), Q.X2.insert(Q.X2.end(), X2, X2 + 3);
        Q.c1.push_back(kf1->use_distort && kf1->cam_of_key ? kf1->cam_of_key[i1] : 0);
        Q.c2.push_back(K2.use_distort && K2.cam_of_key ? K2.cam_of_key[i2] : 0);
      }
    }
    if (samples) smp.insert(smp.end(), samples + (size_t)c * n_rows * 3, samples + (size_t)(c + 1) * n_rows * 3);
  }
  memset(result, 0, sizeof(*result));
  result->cand = -1;
  std::fill(match12, match12 + N1, -1);
  result->n_visits = n_visits;
  auto finish = [&]() -> int {
    result->n_visits = n_visits;
    if (n_visits > trace_capacity) {
      set_error("ComputeSim3: %d visits, the trace holds %d", n_visits, trace_capacity);
      return VIEO_E_CAPACITY;
    }
    return VIEO_OK;
  };
  if (nCandidates == 0) return finish();
  std::vector<vieo_sim3_candidate> sc;
  for (Corr& Q : corr) {
    vieo_sim3_candidate s;
    memset(&s, 0, sizeof(s));
    s.n = (int32_t)Q.i1.size(), s.n1 = N1;
    s.X1 = Q.X1.data(), s.X2 = Q.X2.data(), s.max_err1 = Q.e1.data(), s.max_err2 = Q.e2.data(), s.index1 = Q.i1.data();
    s.cam1 = Q.c1.data(), s.cam2 = Q.c2.data(), s.cams1 = cams1.data(), s.cams2 = Q.cams2.data();
    s.n_cams1 = (int32_t)cams1.size(), s.n_cams2 = (int32_t)Q.cams2.size(), s.fix_scale = fix_scale != 0;
    sc.push_back(s);
  }
  const vieo_sim3_params par{0.99, min_inliers, 300};
  vieo_sim3_solver* solver = nullptr;
  rc = vieo_sim3_create(&solver, sc.data(), nCandidates, &par, samples ? smp.data() : nullptr, n_rows, seed);
  if (rc != VIEO_OK) return rc;
  // ---- 3. the while: per pass the look-ups, one SearchBySim3, one OptimizeSim3, then the decisions in candidate order
  struct Pass {
    vieo_compute_sim3_visit line;
    int visit;  // index into the pass's search / optimise visits, -1: no Sim3
  };
  std::vector<Pass> pass;
  std::vector<std::vector<int32_t>> m12;
  std::vector<vieo_sim3_visit> sv;
  std::vector<vieo_sim3_opt_visit> ov;
  std::vector<uint8_t> inl(std::max(N1, 1));
  bool bMatch = false;
  while (nCandidates > 0 && !bMatch && rc == VIEO_OK) {
    pass.clear(), sv.clear(), ov.clear();
    m12.clear();
    m12.reserve(n_cands);
    for (int c = 0; c < n_cands && rc == VIEO_OK; c++) {
      if (discarded[c]) continue;
      Pass P{blank, -1};
      P.line.cand = c, P.line.call = ++calls[c];
      int32_t found = 0, nInliers = 0, bNoMore = 0, row = -1;
      float T12[16];
      rc = vieo_sim3_iterate(solver, solver_of[c], 5, &found, T12, inl.data(), &nInliers, &bNoMore, &row);
      if (rc == VIEO_E_CAPACITY) rc = VIEO_OK, found = 0, bNoMore = 2;  // the sample table is used up: no more draws
      if (rc != VIEO_OK) break;
      P.line.row = row, P.line.no_more = bNoMore, P.line.found = found, P.line.n_inliers = nInliers;
      if (bNoMore) discarded[c] = 1, nCandidates--;
      if (found) {
        vieo_sim3_visit V;
        memset(&V, 0, sizeof(V));
        V.kf2 = c;
        if ((rc = vieo_sim3_get_estimate(solver, solver_of[c], V.R12, V.t12, &V.s12)) != VIEO_OK) break;
        const int32_t* m = &match[(size_t)c * N1];
        m12.emplace_back(N1);
        for (int j = 0; j < N1; j++) m12.back()[j] = inl[j] ? m[j] : -1;
        P.visit = (int)sv.size();
        sv.push_back(V);
      }
      pass.push_back(P);
    }
    if (rc != VIEO_OK) break;
    if (!sv.empty()) {
      for (size_t k = 0; k < sv.size(); k++) sv[k].match12 = m12[k].data();
      if ((rc = vieo_search_by_sim3(kf1, cands, n_cands, sv.data(), (int)sv.size(), 7.5f)) != VIEO_OK) break;
      ov.resize(sv.size());
      for (size_t k = 0; k < sv.size(); k++) {  // g2o::Sim3 gScm(toMatrix3d(R), toVector3d(t), s)
        vieo_sim3_opt_visit& O = ov[k];
        memset(&O, 0, sizeof(O));
        O.kf2 = sv[k].kf2, O.s12 = (double)sv[k].s12, O.match12 = m12[k].data();
        for (int i = 0; i < 9; i++) O.R12[i] = (double)sv[k].R12[i];
        for (int i = 0; i < 3; i++) O.t12[i] = (double)sv[k].t12[i];
      }
      if ((rc = vieo_optimize_sim3(kf1, cands, n_cands, ov.data(), (int)ov.size(), 10.f, fix_scale != 0)) != VIEO_OK) break;
    }
    for (const Pass& P : pass) {
      vieo_compute_sim3_visit v = P.line;
      if (P.visit >= 0) v.n_found = sv[P.visit].n_found, v.n_opt_inliers = ov[P.visit].n_inliers;
      visit(v);
      if (P.visit >= 0 && ov[P.visit].n_inliers >= 20) {
        // ---- 4. mg2oScw = gScm * gSmw, gSmw = (R2w, t2w, 1)
        const vieo_sim3_opt_visit& O = ov[P.visit];
        const vieo_loop_keyframe& K2 = cands[v.cand];
        bMatch = true;
        result->found = 1, result->cand = v.cand, result->n_inliers = O.n_inliers, result->s = O.s12;
        for (int r = 0; r < 3; r++) {
          for (int k = 0; k < 3; k++)
            result->R[r * 3 + k] = (O.R12[r * 3] * (double)K2.Rcw[k] + O.R12[r * 3 + 1] * (double)K2.Rcw[3 + k]) + O.R12[r * 3 + 2] * (double)K2.Rcw[6 + k];
          const double Rt = (O.R12[r * 3] * (double)K2.tcw[0] + O.R12[r * 3 + 1] * (double)K2.tcw[1]) + O.R12[r * 3 + 2] * (double)K2.tcw[2];
          result->t[r] = O.s12 * Rt + O.t12[r];
        }
        for (int r = 0; r < 3; r++) {
          for (int k = 0; k < 3; k++) result->Scw[r * 4 + k] = (float)(result->s * result->R[r * 3 + k]);
          result->Scw[r * 4 + 3] = (float)result->t[r];
        }
        memcpy(match12, m12[P.visit].data(), (size_t)N1 * 4);
        break;
      }
    }
  }
  vieo_sim3_destroy(solver);
  if (rc != VIEO_OK) return rc;
  return finish();
}
