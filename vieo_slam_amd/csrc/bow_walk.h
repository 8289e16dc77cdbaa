// bow_walk.h -- the host half of the searches that walk two DBoW2::FeatureVectors (bow_search.hip, tri_search.hip):
// the check of a node table, the enumeration of the nodes two vectors share, the rotation histogram with its
// erasures, and, for both SearchByBoW forms, the query plan the device computes distances for and the walk over those
// distances, which depends on its own earlier matches.  Host-only C++ (no HIP): the tests compile it with g++
// (tests/emul/bow_walk_emul.cc, tests/test_bow_walk.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <unordered_map>
#include <vector>

#include "../../include/vieo_hot.h"
#include "orb_match.h"

namespace vieo {

void set_error(const char* fmt, ...);

// mFeatVec as node_id[n_nodes] / node_first[n_nodes + 1] / node_feat: the arrays are there, the ids ascend, node_first
// starts at 0 and does not decrease, every feature index is a key
static inline bool node_table_ok(int n_keys, int n_nodes, const uint32_t* node_id, const int32_t* node_first, const int32_t* node_feat) {
  if (n_nodes <= 0) return n_nodes == 0;
  if (!node_id || !node_first || node_first[0] != 0) return false;
  for (int n = 0; n < n_nodes; n++)
    if (node_first[n + 1] < node_first[n] || (n > 0 && node_id[n] <= node_id[n - 1])) return false;
  if (node_first[n_nodes] > 0 && !node_feat) return false;
  for (int i = 0; i < node_first[n_nodes]; i++)
    if (node_feat[i] < 0 || node_feat[i] >= n_keys) return false;
  return true;
}

// The reference's walk over two FeatureVectors (e.g. ORBmatcher.cc:365-372, :496-503): body(a, b) for every pair of
// entries with one node id, ascending; otherwise lower_bound on the side that is behind.
template <class Body>
static inline void for_shared_nodes(const uint32_t* id_a, int n_a, const uint32_t* id_b, int n_b, Body&& body) {
  int a = 0, b = 0;
  while (a < n_a && b < n_b) {
    if (id_a[a] == id_b[b]) {
      body(a, b);
      a++, b++;
    } else if (id_a[a] < id_b[b])
      a = (int)(std::lower_bound(id_a + a, id_a + n_a, id_b[b]) - id_a);
    else
      b = (int)(std::lower_bound(id_b + b, id_b + n_b, id_a[a]) - id_b);
  }
}

// rotHist with rothist2erase: a pushed key (>= 0) keeps its (bin, position) until finish
struct RotHist {
  std::vector<int> bins[kHistoLen];
  size_t push(int bin, int key) { return bins[bin].push_back(key), bins[bin].size() - 1; }
  void erase(int bin, size_t pos) { bins[bin][pos] = -1; }
  // ComputeThreeMaxima over what was not erased; drop(key) for every surviving key of a losing bin
  template <class Drop>
  void finish(Drop&& drop) {
    int count[kHistoLen];
    for (int i = 0; i < kHistoLen; i++) {
      bins[i].erase(std::remove(bins[i].begin(), bins[i].end(), -1), bins[i].end());
      count[i] = (int)bins[i].size();
    }
    const unsigned losers = three_maxima(count);
    for (int i = 0; i < kHistoLen; i++)
      if ((losers >> i) & 1u)
        for (int key : bins[i]) drop(key);
  }
};

// ---- the two SearchByBoW forms.  A query is a key of the LEFT side that holds a map point and sits in a node the
// RIGHT side shares; its distances are to the node's keys of the right side, in the node's order.
//   SearchByBoW(KeyFrame*, Frame&):      left = the key frame, right = the frame, match[] over the frame's keys
//   SearchByBoW(KeyFrame*, KeyFrame*):   left = pKF1, right = the candidate pKF2, match[] over pKF1's keys
struct BowQuery {
  int desc, first_f, count_f, out_off;  // the key's descriptor (index into the concatenated array), the node's run in the
};                                      // device's feature list, where its count_f distances go

struct BowPlan {  // the queries of n pairs in the reference's order: shared nodes ascending, the left keys in the node's order
  std::vector<BowQuery> queries;
  std::vector<int> key;        // [query] the left key
  std::vector<int> q_begin;    // [n + 1] the queries of pair p
  std::vector<int> feat_base;  // [n] where the right side's node_feat lies in the device's feature list
  std::vector<int> feat;       // key-frame form: the candidates' node_feat lists, each entry moved to its descriptor
  size_t n_dist = 0;
  // the right side's keys of query q of pair p
  const int32_t* run(int p, int q, const vieo_bow_keys& right) const { return right.node_feat + (queries[q].first_f - feat_base[p]); }
};

static inline void bow_plan_pair(const vieo_bow_keys& left, int left_desc, const vieo_bow_keys& right, int feat_base, BowPlan& P) {
  P.q_begin.push_back((int)P.queries.size());
  P.feat_base.push_back(feat_base);
  for_shared_nodes(left.node_id, left.n_nodes, right.node_id, right.n_nodes, [&](int nl, int nr) {
    const int first = right.node_first[nr], count = right.node_first[nr + 1] - first;
    for (int i = left.node_first[nl]; i < left.node_first[nl + 1] && count > 0; i++) {
      const int idx = left.node_feat[i];
      if (left.mp_id[idx] < 0) continue;
      P.queries.push_back(BowQuery{left_desc + idx, feat_base + first, count, (int)P.n_dist});
      P.key.push_back(idx);
      P.n_dist += count;
    }
  });
}

// descriptors: the frame's, then those of the key frames; feature list: the frame's node_feat
static inline BowPlan bow_plan_frame(const vieo_bow_keys& F, const vieo_bow_keys* kfs, int n_kfs) {
  BowPlan P;
  int keys_all = F.n_keys;
  for (int p = 0; p < n_kfs; keys_all += kfs[p].n_keys, p++) bow_plan_pair(kfs[p], keys_all, F, 0, P);
  P.q_begin.push_back((int)P.queries.size());
  return P;
}

// descriptors: pKF1's, then those of the candidates; feature list: P.feat
static inline BowPlan bow_plan_kf(const vieo_bow_keys& A, const vieo_bow_keys* kf2s, int n_kf2) {
  BowPlan P;
  int keys_all = A.n_keys;
  for (int p = 0; p < n_kf2; keys_all += kf2s[p].n_keys, p++) {
    const vieo_bow_keys& B = kf2s[p];
    const int feat_base = (int)P.feat.size();
    for (int i = 0; i < (B.n_nodes ? B.node_first[B.n_nodes] : 0); i++) P.feat.push_back(keys_all + B.node_feat[i]);
    bow_plan_pair(A, 0, B, feat_base, P);
  }
  P.q_begin.push_back((int)P.queries.size());
  return P;
}

// The order-dependent walk of SearchByBoW(KeyFrame*, Frame&) for key frame p of the plan (ORBmatcher.cc:365-502), the
// rectified form (key_cam == nullptr: F.mapn2in_ is empty, every key is of image 0) and the per-image one
// (key_cam[j] = get<0>(F.mapn2in_[j]) < 4) in one.  match[F.n_keys]: the key-frame key whose map point a frame key got.
// Where it differs from bow_walk_kf is marked (a) .. (e) in both.
static inline int bow_walk_frame(const BowPlan& P, int p, const uint16_t* dist, const vieo_bow_keys& B, const vieo_bow_keys& F,
                          const uint8_t* key_cam, float nn_ratio, int check_orientation, int32_t* match, int32_t* n_matches) {
  struct Held { int dist, idx_f, bin; size_t pos; };  // mapmpcami2distkpidhist
  std::fill(match, match + F.n_keys, -1);
  RotHist rot;
  std::unordered_map<uint64_t, Held> held;  // (c) keyed by (map point, image): the id, then the image in 2 bits
  int nmatches = 0;
  for (int q = P.q_begin[p]; q < P.q_begin[p + 1]; q++) {
    const BowQuery& Q = P.queries[q];
    const int idx_kf = P.key[q];
    const int32_t* run = P.run(p, q, F);
    // (b) vbestDist1 / vbestDist2 / vbestIdxF per image: slot img exists once a key of an image >= img has been looked
    // at; frame keys already matched are skipped
    int best1[4] = {256, 256, 256, 256}, best2[4] = {256, 256, 256, 256}, best_f[4] = {-1, -1, -1, -1}, n_slots = 1;
    for (int k = 0; k < Q.count_f; k++) {
      const int idx_f = run[k];
      if (match[idx_f] != -1) continue;
      const int d = dist[Q.out_off + k];
      const int img = key_cam ? key_cam[idx_f] : 0;
      if (n_slots <= img) n_slots = img + 1;
      if (d < best1[img])
        best2[img] = best1[img], best1[img] = d, best_f[img] = idx_f;
      else if (d < best2[img])
        best2[img] = d;
    }
    const int32_t mp = B.mp_id[idx_kf];
    for (int img = 0; img < n_slots; img++) {
      if (best1[img] > kThLow) continue;  // (a) bestDist1 <= TH_LOW passes
      if (!((float)best1[img] < nn_ratio * (float)best2[img])) continue;
      const uint64_t mpcami = ((uint64_t)(uint32_t)mp << 2) | (uint64_t)img;
      auto it = held.find(mpcami);
      if (it != held.end()) {
        if (it->second.dist <= best1[img]) continue;
        match[it->second.idx_f] = -1;  // (e) nothing else to restore
        --nmatches;
        if (check_orientation) rot.erase(it->second.bin, it->second.pos);
      }
      match[best_f[img]] = idx_kf;
      Held h{best1[img], best_f[img], -1, 0};
      if (check_orientation) {
        h.bin = rot_bin(B.keys[idx_kf].angle, F.keys[best_f[img]].angle);
        if (h.bin < 0 || h.bin >= kHistoLen) {
          set_error("SearchByBoW: key angles outside [0, 360)");
          return VIEO_E_INVALID;
        }
        h.pos = rot.push(h.bin, best_f[img]);
      }
      held.emplace(mpcami, h);  // (d) never overwritten once emplaced, as in the reference
      nmatches++;
    }
  }
  if (check_orientation) rot.finish([&](int idx_f) { match[idx_f] = -1, nmatches--; });
  *n_matches = nmatches;
  return VIEO_OK;
}

// The order-dependent walk of SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2) for candidate p of the plan
// (ORBmatcher.cc:753-891).  match12[A.n_keys]: the candidate's key a key of pKF1 got.
static inline int bow_walk_kf(const BowPlan& P, int p, const uint16_t* dist, const vieo_bow_keys& A, const vieo_bow_keys& B,
                       float nn_ratio, int check_orientation, int32_t* match12, int32_t* n_matches) {
  struct Held { int dist, idx1, idx2, bin; size_t pos; };  // mapmpcami2distkp12idhist
  std::fill(match12, match12 + A.n_keys, -1);
  std::vector<uint8_t> matched2(B.n_keys, 0);
  RotHist rot;
  std::unordered_map<int32_t, Held> held;  // (c) keyed by pKF1's map point
  int nmatches = 0;
  for (int q = P.q_begin[p]; q < P.q_begin[p + 1]; q++) {
    const BowQuery& Q = P.queries[q];
    const int idx1 = P.key[q];
    const int32_t* run = P.run(p, q, B);
    // (b) one best / second best, over the candidate's keys that hold a map point and are not in matched2
    int best1 = 256, best2 = 256, best_idx2 = -1;
    for (int k = 0; k < Q.count_f; k++) {
      const int idx2 = run[k];
      if (matched2[idx2] || B.mp_id[idx2] < 0) continue;
      const int d = dist[Q.out_off + k];
      if (d < best1)
        best2 = best1, best1 = d, best_idx2 = idx2;
      else if (d < best2)
        best2 = d;
    }
    if (!(best1 < kThLow)) continue;  // (a) bestDist1 < TH_LOW passes, TH_LOW itself does not
    if (!((float)best1 < nn_ratio * (float)best2)) continue;
    const int32_t mp = A.mp_id[idx1];
    auto it = held.find(mp);
    if (it != held.end()) {
      if (it->second.dist <= best1) continue;
      match12[it->second.idx1] = -1;
      matched2[it->second.idx2] = 0;  // (e) the replaced entry's key of pKF2 is free again
      --nmatches;
      if (check_orientation) rot.erase(it->second.bin, it->second.pos);
    }
    match12[idx1] = best_idx2;
    matched2[best_idx2] = 1;
    Held h{best1, idx1, best_idx2, -1, 0};
    if (check_orientation) {
      h.bin = rot_bin(A.keys[idx1].angle, B.keys[best_idx2].angle);
      if (h.bin < 0 || h.bin >= kHistoLen) {
        set_error("SearchByBoW(KF, KF): key angles outside [0, 360)");
        return VIEO_E_INVALID;
      }
      h.pos = rot.push(h.bin, idx1);
    }
    held.emplace(mp, h);  // (d) never overwritten once emplaced, as in the reference
    nmatches++;
  }
  if (check_orientation) rot.finish([&](int idx1) { match12[idx1] = -1, nmatches--; });
  *n_matches = nmatches;
  return VIEO_OK;
}

}  // namespace vieo
