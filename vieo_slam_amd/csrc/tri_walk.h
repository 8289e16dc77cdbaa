// tri_walk.h -- what tri_search.hip does on the host between its launches: the argument checks of its three entries,
// the plan (where every key frame lies in the concatenated device arrays, and the queries of k_tri_gates in the
// reference's order), the order-dependent walk of SearchForTriangulation over the candidates the kernel kept
// (ORBmatcher.cc:962-1146), and the row gather / result scatter around k_tri_new_points (LocalMapping.cc:691-698).
// Host-only C++ (no HIP): the tests compile it with g++ (tests/emul/tri_walk_emul.cc, tests/test_tri_walk.py).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/vieo_hot.h"
#include "bow_walk.h"
#include "match_groups.h"

namespace vieo {

// the arguments of the three entries and which halves the entry runs; what an entry does not take stays null or 0
// (filled member by member from TriArgs{}, never positionally)
struct TriArgs {
  bool search, tri;
  const vieo_tri_keyframe *kf1, *kf2s;
  const vieo_tri_stereo *st1, *st2s;
  int n_kf2, only_stereo, check_orientation;
  float th_far_pts;
  int32_t pair_capacity, pair_stride;
  int32_t *h_pairs, *h_n_pairs, *h_n_matches;  // what the search writes
  const int32_t *rows, *n_rows;                // what the triangulation reads: the caller's rows, or h_pairs / h_n_pairs
  int8_t* h_status;
  double* h_x3d;
  float* h_x3d_f;
  int32_t* h_n_new;
  const vieo_tri_keyframe& kf(int f) const { return f == 0 ? *kf1 : kf2s[f - 1]; }  // 0 = pKF1, 1 + p = neighbour p
  const vieo_tri_stereo& st(int f) const { return f == 0 ? *st1 : st2s[f - 1]; }
};

struct TriQuery {  // a key of pKF1 against the keys of one shared node of neighbour `pair`
  int idx1, pair, first2, count2, out_off;
};
struct TriCand {  // what k_tri_gates keeps of a query's run, in the run's order
  int idx2, dist;
};

static inline int tri_cams(const vieo_tri_keyframe& K) { return K.n_cams > 0 ? K.n_cams : 1; }

// the baseline test of LocalMapping.cc:691-698 (stereo / RGB-D / rigs)
static inline bool tri_baseline_short(const vieo_tri_stereo& s1, const vieo_tri_stereo& s2) {
  const float v[3] = {s2.Ow[0] - s1.Ow[0], s2.Ow[1] - s1.Ow[1], s2.Ow[2] - s1.Ow[2]};
  return std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) < s2.baseline;
}

// ---- checks.  cam_ok: the camera model's own check, which the device side owns
static inline bool tri_kf_ok(const vieo_tri_keyframe& K, bool (*cam_ok)(const vieo_camera&)) {
  if (K.n_keys < 0 || K.n_nodes < 0 || K.n_levels <= 0 || !K.scale_factor || !K.level_sigma2) return false;
  if (K.n_keys > 0 && (!K.keys || !K.descriptors || !K.uright || !K.has_mappoint)) return false;
  if (K.n_cams < 0 || K.n_cams > 4 || (K.n_cams > 0 && (!K.cams || !K.Tcr || !K.Trc || (K.n_keys > 0 && !K.key_cam)))) return false;
  if (!node_table_ok(K.n_keys, K.n_nodes, K.node_id, K.node_first, K.node_feat)) return false;
  for (int i = 0; i < K.n_keys; i++)
    if (K.keys[i].octave < 0 || K.keys[i].octave >= K.n_levels || (K.n_cams > 0 && K.key_cam[i] >= K.n_cams)) return false;
  for (int c = 0; c < K.n_cams; c++)
    if (!cam_ok(K.cams[c])) return false;
  return true;
}

static inline bool tri_stereo_ok(const vieo_tri_keyframe& K, const vieo_tri_stereo& S, int* n_groups) {
  if (K.n_keys > 0 && !S.depth) return false;
  if (K.n_cams > 0 && S.key_group)
    for (int i = 0; i < K.n_keys; i++) {
      if (S.key_group[i] < -1) return false;
      *n_groups = std::max(*n_groups, S.key_group[i] + 1);
    }
  return *n_groups == 0 || S.group_p3d;
}

// VIEO_OK with n_kf2 == 0: a key frame without neighbours, nothing to do.  n_groups[f]: the groups of key frame f
static inline int tri_check(const TriArgs& a, bool (*cam_ok)(const vieo_camera&), std::vector<int>& n_groups) {
  const bool tri = a.tri;  // else the search alone
  if (!a.kf1 || a.n_kf2 < 0 || a.pair_capacity < 0 || (tri ? !a.st1 : a.n_kf2 == 0)) return VIEO_E_INVALID;
  if (a.n_kf2 == 0) return VIEO_OK;
  const bool cap = a.pair_capacity > 0;
  if (!a.kf2s || (a.search && (!a.h_n_pairs || !a.h_n_matches || (cap && !a.h_pairs)))) return VIEO_E_INVALID;
  if (tri && (!a.st2s || !a.n_rows || !a.h_n_new || (cap && (!a.rows || !a.h_status || !a.h_x3d || !a.h_x3d_f)))) return VIEO_E_INVALID;
  const char* who = tri ? "CreateNewMapPoints" : "SearchForTriangulation";
  n_groups.assign(1 + a.n_kf2, 0);
  if (!tri_kf_ok(*a.kf1, cam_ok) || (tri && !tri_stereo_ok(*a.kf1, *a.st1, &n_groups[0]))) {
    set_error(tri ? "%s: pKF1 is inconsistent"
                  : "%s: pKF1 is inconsistent (nodes ascending, feature / camera indices and octaves in range)", who);
    return VIEO_E_INVALID;
  }
  for (int p = 0; p < a.n_kf2; p++) {
    const vieo_tri_keyframe& B = a.kf2s[p];
    if (!tri_kf_ok(B, cam_ok) || (tri && !tri_stereo_ok(B, a.st2s[p], &n_groups[1 + p]))) {
      set_error("%s: neighbour %d is inconsistent", who, p);
      return VIEO_E_INVALID;
    }
    if ((B.n_cams > 0) != (a.kf1->n_cams > 0)) {  // assert(!usedistort[1]) / assert(usedistort[1]), ORBmatcher.cc:949,952
      set_error("%s: neighbour %d and pKF1 are not of one kind (undistorted / rig)", who, p);
      return VIEO_E_INVALID;
    }
    if (a.pair_stride < tri_cams(*a.kf1) + tri_cams(B)) {
      set_error("%s: pair_stride %d is smaller than the cameras of pair %d", who, a.pair_stride, p);
      return VIEO_E_INVALID;
    }
  }
  return VIEO_OK;
}

// ---- the plan.  Every per-key (per-feature, per-level, per-group) device array holds pKF1's part, then the
// neighbours' in call order: part f starts at *_off[f], *_off[1 + n_kf2] is the total.  Computed once per call; the
// search and the triangulation both read it.
struct TriPlan {
  std::vector<int> key_off, feat_off, lvl_off, group_off;  // feat: the neighbours' node_feat lists (pKF1's part is empty)
  int max_keys = 1;
  std::vector<TriQuery> queries;  // shared nodes ascending, pKF1's keys in the node's order; of neighbour p: q_begin[p] ...
  std::vector<int> q_begin;
  size_t n_cand = 0;  // the runs of all queries, one after the other at out_off
};

static inline void tri_layout(const TriArgs& a, const std::vector<int>& n_groups, TriPlan& P) {
  const int nf = 1 + a.n_kf2;
  P.key_off.assign(nf + 1, 0), P.feat_off.assign(nf + 1, 0), P.lvl_off.assign(nf + 1, 0), P.group_off.assign(nf + 1, 0);
  P.max_keys = 1, P.queries.clear(), P.q_begin.assign(a.n_kf2 + 1, 0), P.n_cand = 0;
  for (int f = 0; f < nf; f++) {
    const vieo_tri_keyframe& K = a.kf(f);
    P.key_off[f + 1] = P.key_off[f] + K.n_keys;
    P.feat_off[f + 1] = P.feat_off[f] + (f > 0 && K.n_nodes ? K.node_first[K.n_nodes] : 0);
    P.lvl_off[f + 1] = P.lvl_off[f] + K.n_levels;
    P.group_off[f + 1] = P.group_off[f] + n_groups[f];
    P.max_keys = std::max(P.max_keys, K.n_keys);
  }
}

// keys of pKF1 with a map point are left out, under only_stereo the monocular ones too; a neighbour closer than its
// stereo baseline (an entry that triangulates) is not searched
static inline void tri_queries(const TriArgs& a, TriPlan& P) {
  const vieo_tri_keyframe& A = *a.kf1;
  for (int p = 0; p < a.n_kf2; p++) {
    const vieo_tri_keyframe& B = a.kf2s[p];
    P.q_begin[p] = (int)P.queries.size();
    if (a.tri && tri_baseline_short(*a.st1, a.st2s[p])) continue;
    for_shared_nodes(A.node_id, A.n_nodes, B.node_id, B.n_nodes, [&](int n1, int n2) {
      const int first2 = B.node_first[n2], count2 = B.node_first[n2 + 1] - first2;
      for (int i1 = A.node_first[n1]; i1 < A.node_first[n1 + 1] && count2 > 0; i1++) {
        const int idx1 = A.node_feat[i1];
        if (A.has_mappoint[idx1] || (a.only_stereo && !(A.uright[idx1] >= 0))) continue;
        P.queries.push_back({idx1, p, first2, count2, (int)P.n_cand});
        P.n_cand += count2;
      }
    });
  }
  P.q_begin[a.n_kf2] = (int)P.queries.size();
}

// ---- the walk of neighbour p (ORBmatcher.cc:962-1146) over cand[Q.out_off ...] / cand_n[q]: rows to h_pairs, the
// row count and the reference's return value.  G: scratch
static inline int tri_walk_pair(const TriArgs& a, const TriPlan& P, int p, const TriCand* cand, const int* cand_n, FeGroups& G) {
  const vieo_tri_keyframe &A = *a.kf1, &B = a.kf2s[p];
  const bool rig = A.n_cams > 0;
  const int nc1 = tri_cams(A), nc2 = tri_cams(B), nc = nc1 + nc2;
  int32_t nk[8];
  for (int c = 0; c < nc; c++) nk[c] = c < nc1 ? A.n_keys : B.n_keys;  // tables indexed by the key's global index
  G.reset(nc, nk);
  RotHist rot;
  int nmatches = 0;
  for (int q = P.q_begin[p]; q < P.q_begin[p + 1]; q++) {
    const TriQuery& Q = P.queries[q];
    const int cam1 = rig ? A.key_cam[Q.idx1] : 0;
    int bestDist[4] = {kThLow, kThLow, kThLow, kThLow}, bestIdx2[4] = {-1, -1, -1, -1};  // per image
    for (int k = 0; k < cand_n[q]; k++) {
      const TriCand c = cand[Q.out_off + k];
      const int img = rig ? B.key_cam[c.idx2] : 0;
      const int g = G.key2g[nc1 + img][c.idx2];
      if (g >= 0 && G.idxs[(size_t)g * nc + cam1] != -1) continue;  // pKF2's key already matched to this camera
      if (c.dist > bestDist[img]) continue;  // ties go to the later key
      bestIdx2[img] = c.idx2, bestDist[img] = c.dist;
    }
    for (int img = 0; img < nc2; img++) {
      if (bestIdx2[img] < 0) continue;
      if (fe_fill(G, cam1, Q.idx1, nc1 + img, bestIdx2[img], (float)bestDist[img])) ++nmatches;
      if (a.check_orientation) {
        const int bin = rot_bin(A.keys[Q.idx1].angle, B.keys[bestIdx2[img]].angle);
        if (bin < 0 || bin >= kHistoLen) {
          set_error("SearchForTriangulation: key angles outside [0, 360)");
          return VIEO_E_INVALID;
        }
        rot.push(bin, Q.idx1);
      }
    }
  }
  if (a.check_orientation)
    rot.finish([&](int idx1) {
      const int g = G.key2g[rig ? A.key_cam[idx1] : 0][idx1];
      if (g < 0) return;
      G.good[g] = 0;
      nmatches--;
    });
  int np = 0;
  for (int g = 0; g < G.size(); g++) {
    int cnt = 0;
    for (int c = 0; c < nc; c++) cnt += G.idxs[(size_t)g * nc + c] != -1;
    if (cnt < 2 || !G.good[g]) continue;
    if (np < a.pair_capacity) {
      int32_t* row = a.h_pairs + ((size_t)p * a.pair_capacity + np) * a.pair_stride;
      for (int c = 0; c < a.pair_stride; c++) row[c] = c < nc ? G.idxs[(size_t)g * nc + c] : -1;
    }
    np++;
  }
  a.h_n_pairs[p] = np, a.h_n_matches[p] = nmatches;
  if (np > a.pair_capacity) {
    set_error("SearchForTriangulation: neighbour %d has %d matches, capacity %d", p, np, a.pair_capacity);
    return VIEO_E_CAPACITY;
  }
  return VIEO_OK;
}

static inline int tri_walk(const TriArgs& a, const TriPlan& P, const TriCand* cand, const int* cand_n) {
  FeGroups G;  // (one allocation for all neighbours)
  for (int p = 0; p < a.n_kf2; p++)
    if (const int rc = tri_walk_pair(a, P, p, cand, cand_n, G)) return rc;
  return VIEO_OK;
}

// ---- the rows k_tri_new_points works on: those of the neighbours that pass the baseline test, one after the other,
// padded to pair_stride; the rows of the others are SKIPPED here
struct TriRows {
  std::vector<int32_t> rows, row_pair;
  std::vector<size_t> row_dst;  // where in h_status / h_x3d / h_x3d_f a row's result goes
  int n() const { return (int)row_pair.size(); }
};

static inline int tri_gather(const TriArgs& a, TriRows& R) {
  const vieo_tri_keyframe& A = *a.kf1;
  const int nc1 = tri_cams(A);
  R.rows.clear(), R.row_pair.clear(), R.row_dst.clear();
  for (int p = 0; p < a.n_kf2; p++) {
    a.h_n_new[p] = 0;
    const int np = a.n_rows[p];
    if (np < 0) {
      set_error("CreateNewMapPoints: neighbour %d has a negative row count", p);
      return VIEO_E_INVALID;
    }
    if (np > a.pair_capacity) {
      set_error("CreateNewMapPoints: neighbour %d has %d rows, capacity %d", p, np, a.pair_capacity);
      return VIEO_E_CAPACITY;
    }
    const vieo_tri_keyframe& B = a.kf2s[p];
    const int nc = nc1 + tri_cams(B);
    const bool skip = tri_baseline_short(*a.st1, a.st2s[p]);
    for (int m = 0; m < np; m++) {
      const size_t at = (size_t)p * a.pair_capacity + m;
      const int32_t* row = a.rows + at * a.pair_stride;
      if (skip) {
        a.h_status[at] = VIEO_NEWPT_SKIPPED;
        for (int q = 0; q < 3; q++) a.h_x3d[at * 3 + q] = 0, a.h_x3d_f[at * 3 + q] = 0;
        continue;
      }
      for (int c = 0; c < nc; c++)
        if (row[c] < -1 || row[c] >= (c < nc1 ? A.n_keys : B.n_keys)) {
          set_error("CreateNewMapPoints: row %d of neighbour %d holds key %d", m, p, row[c]);
          return VIEO_E_INVALID;
        }
      for (int c = 0; c < a.pair_stride; c++) R.rows.push_back(c < nc ? row[c] : -1);
      R.row_pair.push_back(p), R.row_dst.push_back(at);
    }
  }
  return VIEO_OK;
}

// the kernel's results of row r to row_dst[r]; h_n_new[p]: the accepted rows of neighbour p
static inline void tri_scatter(const TriArgs& a, const TriRows& R, const int8_t* st, const double* x3d, const float* x3d_f) {
  for (int r = 0; r < R.n(); r++) {
    const size_t at = R.row_dst[r];
    a.h_status[at] = st[r];
    for (int q = 0; q < 3; q++) a.h_x3d[at * 3 + q] = x3d[(size_t)r * 3 + q], a.h_x3d_f[at * 3 + q] = x3d_f[(size_t)r * 3 + q];
    a.h_n_new[R.row_pair[r]] += st[r] >= 0;
  }
}

}  // namespace vieo
