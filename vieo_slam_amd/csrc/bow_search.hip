// bow_search.hip -- ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) (reference src/ORBmatcher.cc:344-505;
// Tracking::Relocalization, Tracking.cc:2554, and TrackReferenceKeyFrame, :1731) for a batch of key frames against one
// frame: vieo_search_by_bow for the rectified configuration (every key is of image 0), vieo_search_by_bow_rig for a
// rig frame (F.mapn2in_ filled: best / second best per image, the MATCH_KNN_IN_EACH_IMG branch); one walk for both,
// and ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12) (:726-905; LoopClosing::ComputeSim3) for one key frame
// against a batch of candidates (vieo_search_by_bow_kf, at the end of the file).
//   k_bow_distances  one lane per "query" = a key of a key frame that holds a map point and sits in a vocabulary node
//                    the frame shares: the Hamming distance to every frame key of that node, all key frames in one
//                    launch (the pair enumeration of tri_search.hip)
//   host             the reference's walk over those distances, which depends on its own earlier matches: frame keys
//                    already matched are skipped, best / second best, TH_LOW, the ratio test, the (map point, image)
//                    table with its histogram erasures, the rotation histogram
// A query's distances are as many as its node has frame keys, so the kernel writes without atomics.
#include <algorithm>
#include <cmath>
#include <unordered_map>
#include <vector>

#include "common.h"

namespace vieo {

static const int kBowThLow = 50, kBowHisto = 30;

struct BowQuery {
  int desc, first_f, count_f, out_off;  // the key's descriptor (index into the concatenated array), the node's frame keys
};

__device__ __forceinline__ int bow_hamming(const uint4* a, const uint4* b) {
  const uint4 a0 = a[0], a1 = a[1], b0 = b[0], b1 = b[1];
  return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
         __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// desc: the frame's descriptors first, then those of the key frames; feat_f: the frame's node_feat
__global__ void __launch_bounds__(64)
k_bow_distances(const BowQuery* __restrict__ queries, int n_queries, const uint8_t* __restrict__ desc,
                const int* __restrict__ feat_f, uint16_t* __restrict__ dist) {
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= n_queries) return;
  const BowQuery Q = queries[q];
  const uint4* d1 = (const uint4*)(desc + 32 * (size_t)Q.desc);
  for (int k = 0; k < Q.count_f; k++)
    dist[Q.out_off + k] = (uint16_t)bow_hamming(d1, (const uint4*)(desc + 32 * (size_t)feat_f[Q.first_f + k]));
}

static bool bow_keys_ok(const vieo_bow_keys& K, bool key_frame) {
  if (K.n_keys < 0 || K.n_nodes < 0) return false;
  if (K.n_keys > 0 && (!K.keys || !K.descriptors || (key_frame && !K.mp_id))) return false;
  if (K.n_nodes > 0 && (!K.node_id || !K.node_first || (K.node_first[K.n_nodes] > 0 && !K.node_feat))) return false;
  if (K.n_nodes > 0 && K.node_first[0] != 0) return false;
  for (int i = 0; i < K.n_keys; i++)  // the rotation histogram's bins (the reference asserts)
    if (!(K.keys[i].angle >= 0.f && K.keys[i].angle < 360.f)) return false;
  for (int n = 0; n < K.n_nodes; n++)
    if (K.node_first[n + 1] < K.node_first[n] || (n > 0 && K.node_id[n] <= K.node_id[n - 1])) return false;
  for (int i = 0; i < (K.n_nodes ? K.node_first[K.n_nodes] : 0); i++)
    if (K.node_feat[i] < 0 || K.node_feat[i] >= K.n_keys) return false;
  return true;
}

static void bow_three_maxima(const std::vector<int>* histo, int L, int& ind1, int& ind2, int& ind3) {  // ORBmatcher.cc:1608-1641
  int max1 = 0, max2 = 0, max3 = 0;
  for (int i = 0; i < L; i++) {
    const int s = (int)histo[i].size();
    if (s > max1)
      max3 = max2, max2 = max1, max1 = s, ind3 = ind2, ind2 = ind1, ind1 = i;
    else if (s > max2)
      max3 = max2, max2 = s, ind3 = ind2, ind2 = i;
    else if (s > max3)
      max3 = s, ind3 = i;
  }
  if (max2 < 0.1f * (float)max1)
    ind2 = -1, ind3 = -1;
  else if (max3 < 0.1f * (float)max1)
    ind3 = -1;
}

struct BowScratch {
  DevBuf q, d, f, out;
};
static thread_local BowScratch g_bow;

// The device part of both entries: the descriptors of `first`, then those of the n `others`, the feature list the
// queries' runs point into, one launch, the distances back.
static int bow_run_distances(const std::vector<BowQuery>& queries, const vieo_bow_keys& first, const vieo_bow_keys* others,
                             int n, const int* feat, size_t n_feat, std::vector<uint16_t>& dist, size_t n_dist) {
  const int nq = (int)queries.size();
  if (nq == 0) return VIEO_OK;
  size_t keys_all = first.n_keys;
  for (int p = 0; p < n; p++) keys_all += others[p].n_keys;
  BowScratch& S = g_bow;
  int rc;
  if ((rc = S.q.ensure(nq * sizeof(BowQuery))) != VIEO_OK || (rc = S.d.ensure(keys_all * 32)) != VIEO_OK ||
      (rc = S.f.ensure(n_feat * 4)) != VIEO_OK || (rc = S.out.ensure(dist.size() * 2)) != VIEO_OK)
    return rc;
  VIEO_HIP_CHECK(hipMemcpy(S.q.p, queries.data(), nq * sizeof(BowQuery), hipMemcpyHostToDevice));
  VIEO_HIP_CHECK(hipMemcpy(S.d.p, first.descriptors, (size_t)first.n_keys * 32, hipMemcpyHostToDevice));
  size_t off = first.n_keys;
  for (int p = 0; p < n; p++) {
    if (others[p].n_keys)
      VIEO_HIP_CHECK(hipMemcpy(S.d.as<uint8_t>() + 32 * off, others[p].descriptors, (size_t)others[p].n_keys * 32, hipMemcpyHostToDevice));
    off += others[p].n_keys;
  }
  VIEO_HIP_CHECK(hipMemcpy(S.f.p, feat, n_feat * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_bow_distances, dim3((nq + 63) / 64), dim3(64), 0, nullptr, S.q.as<BowQuery>(), nq,
                     S.d.as<uint8_t>(), S.f.as<int>(), S.out.as<uint16_t>());
  VIEO_HIP_CHECK(hipGetLastError());
  VIEO_HIP_CHECK(hipMemcpy(dist.data(), S.out.p, n_dist * 2, hipMemcpyDeviceToHost));
  return VIEO_OK;
}

}  // namespace vieo

namespace vieo {

// Both SearchByBoW(KeyFrame*, Frame&) entries.  key_cam == nullptr: F.mapn2in_ is empty, every key is of image 0 and
// there is one best / second best; otherwise key_cam[j] = get<0>(F.mapn2in_[j]) and they are kept per image.
static int bow_search_frame(const vieo_bow_keys* frame, const uint8_t* key_cam, const vieo_bow_keys* kfs, int n_kfs,
                            float nn_ratio, int check_orientation, int32_t* h_match, int32_t* h_n_matches) {
  if (!frame || !kfs || n_kfs <= 0 || !h_n_matches || (frame->n_keys > 0 && !h_match)) return VIEO_E_INVALID;
  const vieo_bow_keys& F = *frame;
  if (!bow_keys_ok(F, false)) {
    set_error("SearchByBoW: the frame is inconsistent (nodes ascending, feature indices in range, key angles in [0, 360))");
    return VIEO_E_INVALID;
  }
  for (int p = 0; p < n_kfs; p++)
    if (!bow_keys_ok(kfs[p], true)) {
      set_error("SearchByBoW: key frame %d is inconsistent", p);
      return VIEO_E_INVALID;
    }
  int rc = require_device();
  if (rc != VIEO_OK) return rc;
  // ---- queries in the reference's order: shared nodes ascending, the key frame's keys in the node's order
  struct HostQuery {
    int idx_kf;
  };
  std::vector<BowQuery> queries;
  std::vector<HostQuery> hq;
  std::vector<int> q_begin(n_kfs + 1, 0);
  size_t keys_all = F.n_keys, n_dist = 0;
  for (int p = 0; p < n_kfs; p++) {
    const vieo_bow_keys& B = kfs[p];
    q_begin[p] = (int)queries.size();
    int nk = 0, nf = 0;
    while (nk < B.n_nodes && nf < F.n_nodes) {
      if (B.node_id[nk] == F.node_id[nf]) {
        const int first_f = F.node_first[nf], count_f = F.node_first[nf + 1] - first_f;
        for (int i = B.node_first[nk]; i < B.node_first[nk + 1] && count_f > 0; i++) {
          const int idx = B.node_feat[i];
          if (B.mp_id[idx] < 0) continue;
          queries.push_back(BowQuery{(int)keys_all + idx, first_f, count_f, (int)n_dist});
          hq.push_back(HostQuery{idx});
          n_dist += count_f;
        }
        nk++, nf++;
      } else if (B.node_id[nk] < F.node_id[nf])
        nk = (int)(std::lower_bound(B.node_id + nk, B.node_id + B.n_nodes, F.node_id[nf]) - B.node_id);
      else
        nf = (int)(std::lower_bound(F.node_id + nf, F.node_id + F.n_nodes, B.node_id[nk]) - F.node_id);
    }
    keys_all += B.n_keys;
  }
  q_begin[n_kfs] = (int)queries.size();
  std::vector<uint16_t> dist(std::max<size_t>(n_dist, 1));
  if ((rc = bow_run_distances(queries, F, kfs, n_kfs, F.node_feat, F.n_nodes ? F.node_first[F.n_nodes] : 0, dist, n_dist)) != VIEO_OK)
    return rc;
  // ---- the order-dependent walk, per key frame (ORBmatcher.cc:365-502)
  struct Held {  // mapmpcami2distkpidhist[(pMP, img_id)]: never overwritten once emplaced, as in the reference
    int dist, idx_f, bin;
    size_t pos;
  };
  const float factor = 1.0f / kBowHisto;
  for (int p = 0; p < n_kfs; p++) {
    const vieo_bow_keys& B = kfs[p];
    int32_t* match = h_match + (size_t)p * F.n_keys;
    std::fill(match, match + F.n_keys, -1);
    std::vector<int> rotHist[kBowHisto];
    std::vector<size_t> rothist2erase[kBowHisto];
    std::unordered_map<uint64_t, Held> held;  // key: the map point's id, then the image (4 cameras: 2 bits)
    int nmatches = 0;
    for (int q = q_begin[p]; q < q_begin[p + 1]; q++) {
      const BowQuery& Q = queries[q];
      const int idx_kf = hq[q].idx_kf;
      // vbestDist1 / vbestDist2 / vbestIdxF: slot img_id exists once a key of an image >= img_id has been looked at
      int best1[4] = {256, 256, 256, 256}, best2[4] = {256, 256, 256, 256}, best_f[4] = {-1, -1, -1, -1}, n_slots = 1;
      for (int k = 0; k < Q.count_f; k++) {
        const int idx_f = F.node_feat[Q.first_f + k];
        if (match[idx_f] != -1) continue;  // avoid duplicate matching in this function
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
        if (best1[img] > kBowThLow || !((float)best1[img] < nn_ratio * (float)best2[img])) continue;
        const uint64_t mpcami = ((uint64_t)(uint32_t)mp << 2) | (uint64_t)img;
        auto it = held.find(mpcami);
        if (it != held.end()) {
          if (it->second.dist <= best1[img]) continue;
          match[it->second.idx_f] = -1;
          --nmatches;
          if (check_orientation) rothist2erase[it->second.bin].push_back(it->second.pos);
        }
        match[best_f[img]] = idx_kf;
        Held h{best1[img], best_f[img], -1, 0};
        if (check_orientation) {
          float rot = B.keys[idx_kf].angle - F.keys[best_f[img]].angle;
          if (rot < 0.0) rot += 360.0f;
          int bin = (int)std::round(rot * factor);
          if (bin == kBowHisto) bin = 0;
          if (bin < 0 || bin >= kBowHisto) {
            set_error("SearchByBoW: key angles outside [0, 360)");
            return VIEO_E_INVALID;
          }
          h.bin = bin, h.pos = rotHist[bin].size();
          rotHist[bin].push_back(best_f[img]);
        }
        held.emplace(mpcami, h);
        nmatches++;
      }
    }
    if (check_orientation) {
      std::vector<int> rotHist2[kBowHisto];
      for (int i = 0; i < kBowHisto; i++) {
        for (size_t j : rothist2erase[i]) rotHist[i][j] = -1;
        for (int v : rotHist[i])
          if (v != -1) rotHist2[i].push_back(v);
      }
      int ind1 = -1, ind2 = -1, ind3 = -1;
      bow_three_maxima(rotHist2, kBowHisto, ind1, ind2, ind3);
      for (int i = 0; i < kBowHisto; i++) {
        if (i == ind1 || i == ind2 || i == ind3) continue;
        for (int v : rotHist2[i]) match[v] = -1, nmatches--;
      }
    }
    h_n_matches[p] = nmatches;
  }
  return VIEO_OK;
}

}  // namespace vieo

extern "C" int vieo_search_by_bow(const vieo_bow_keys* frame, const vieo_bow_keys* kfs, int n_kfs, float nn_ratio,
                                  int check_orientation, int32_t* h_match, int32_t* h_n_matches) {
  return vieo::bow_search_frame(frame, nullptr, kfs, n_kfs, nn_ratio, check_orientation, h_match, h_n_matches);
}

extern "C" int vieo_search_by_bow_rig(const vieo_bow_keys* frame, const uint8_t* key_cam, int n_cams,
                                      const vieo_bow_keys* kfs, int n_kfs, float nn_ratio, int check_orientation,
                                      int32_t* h_match, int32_t* h_n_matches) {
  using namespace vieo;
  if (!frame || frame->n_keys < 0 || (frame->n_keys > 0 && !key_cam)) return VIEO_E_INVALID;
  if (n_cams < 1 || n_cams > 4) {
    set_error("SearchByBoW: %d cameras, 1..4", n_cams);
    return VIEO_E_INVALID;
  }
  for (int j = 0; j < frame->n_keys; j++)
    if (key_cam[j] >= n_cams) {
      set_error("SearchByBoW: key %d is of image %d, the frame has %d", j, (int)key_cam[j], n_cams);
      return VIEO_E_INVALID;
    }
  static const uint8_t none = 0;  // (a frame without keys: the walk reads no entry)
  return bow_search_frame(frame, frame->n_keys > 0 ? key_cam : &none, kfs, n_kfs, nn_ratio, check_orientation, h_match,
                          h_n_matches);
}

// ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vpMatches12) (reference src/ORBmatcher.cc:726-905;
// LoopClosing::ComputeSim3, LoopClosing.cc:338) of one key frame against a batch of candidates.  The distances come
// from k_bow_distances as it is: the right-hand side of a query is a run of one feature list, so the candidates'
// node_feat lists are concatenated with each entry moved by its candidate's place in the descriptor array (kf1's
// descriptors first, then those of the candidates).
extern "C" int vieo_search_by_bow_kf(const vieo_bow_keys* kf1, const vieo_bow_keys* kf2s, int n_kf2, float nn_ratio,
                                     int check_orientation, int32_t* h_match12, int32_t* h_n_matches) {
  using namespace vieo;
  if (!kf1 || !kf2s || n_kf2 <= 0 || !h_n_matches || (kf1->n_keys > 0 && !h_match12)) return VIEO_E_INVALID;
  const vieo_bow_keys& A = *kf1;
  if (!bow_keys_ok(A, true)) {
    set_error("SearchByBoW(KF, KF): the key frame is inconsistent (nodes ascending, feature indices in range, key angles in [0, 360))");
    return VIEO_E_INVALID;
  }
  for (int p = 0; p < n_kf2; p++)
    if (!bow_keys_ok(kf2s[p], true)) {
      set_error("SearchByBoW(KF, KF): candidate %d is inconsistent", p);
      return VIEO_E_INVALID;
    }
  int rc = require_device();
  if (rc != VIEO_OK) return rc;
  // ---- queries in the reference's order: shared nodes ascending, kf1's keys in the node's order
  struct HostQuery {
    int idx1, first2;  // the key of kf1; the node's first entry in the candidate's own node_feat
  };
  std::vector<BowQuery> queries;
  std::vector<HostQuery> hq;
  std::vector<int> q_begin(n_kf2 + 1, 0), feat;
  size_t keys_all = A.n_keys, n_dist = 0;
  for (int p = 0; p < n_kf2; p++) {
    const vieo_bow_keys& B = kf2s[p];
    q_begin[p] = (int)queries.size();
    const int feat_base = (int)feat.size();
    for (int i = 0; i < (B.n_nodes ? B.node_first[B.n_nodes] : 0); i++) feat.push_back((int)keys_all + B.node_feat[i]);
    int n1 = 0, n2 = 0;
    while (n1 < A.n_nodes && n2 < B.n_nodes) {
      if (A.node_id[n1] == B.node_id[n2]) {
        const int first2 = B.node_first[n2], count2 = B.node_first[n2 + 1] - first2;
        for (int i = A.node_first[n1]; i < A.node_first[n1 + 1] && count2 > 0; i++) {
          const int idx1 = A.node_feat[i];
          if (A.mp_id[idx1] < 0) continue;
          queries.push_back(BowQuery{idx1, feat_base + first2, count2, (int)n_dist});
          hq.push_back(HostQuery{idx1, first2});
          n_dist += count2;
        }
        n1++, n2++;
      } else if (A.node_id[n1] < B.node_id[n2])
        n1 = (int)(std::lower_bound(A.node_id + n1, A.node_id + A.n_nodes, B.node_id[n2]) - A.node_id);
      else
        n2 = (int)(std::lower_bound(B.node_id + n2, B.node_id + B.n_nodes, A.node_id[n1]) - B.node_id);
    }
    keys_all += B.n_keys;
  }
  q_begin[n_kf2] = (int)queries.size();
  std::vector<uint16_t> dist(std::max<size_t>(n_dist, 1));
  if ((rc = bow_run_distances(queries, A, kf2s, n_kf2, feat.data(), feat.size(), dist, n_dist)) != VIEO_OK) return rc;
  // ---- the order-dependent walk, per candidate (ORBmatcher.cc:753-891)
  struct Held {  // mapmpcami2distkp12idhist[(pMP1, 0)]: never overwritten once emplaced, as in the reference
    int dist, idx1, idx2, bin;
    size_t pos;
  };
  const float factor = 1.0f / kBowHisto;
  for (int p = 0; p < n_kf2; p++) {
    const vieo_bow_keys& B = kf2s[p];
    int32_t* match12 = h_match12 + (size_t)p * A.n_keys;
    std::fill(match12, match12 + A.n_keys, -1);
    std::vector<uint8_t> matched2(B.n_keys, 0);
    std::vector<int> rotHist[kBowHisto];
    std::vector<size_t> rothist2erase[kBowHisto];
    std::unordered_map<int32_t, Held> held;
    int nmatches = 0;
    for (int q = q_begin[p]; q < q_begin[p + 1]; q++) {
      const BowQuery& Q = queries[q];
      const int idx1 = hq[q].idx1;
      int best1 = 256, best2 = 256, best_idx2 = -1;
      for (int k = 0; k < Q.count_f; k++) {
        const int idx2 = B.node_feat[hq[q].first2 + k];
        if (matched2[idx2] || B.mp_id[idx2] < 0) continue;  // avoid duplications; pKF2->mvpMapPoints[idx2] must exist
        const int d = dist[Q.out_off + k];
        if (d < best1)
          best2 = best1, best1 = d, best_idx2 = idx2;
        else if (d < best2)
          best2 = d;
      }
      if (!(best1 < kBowThLow) || !((float)best1 < nn_ratio * (float)best2)) continue;
      const int32_t mp = A.mp_id[idx1];
      auto it = held.find(mp);
      if (it != held.end()) {
        if (it->second.dist <= best1) continue;
        match12[it->second.idx1] = -1;
        matched2[it->second.idx2] = 0;
        --nmatches;
        if (check_orientation) rothist2erase[it->second.bin].push_back(it->second.pos);
      }
      match12[idx1] = best_idx2;
      matched2[best_idx2] = 1;
      Held h{best1, idx1, best_idx2, -1, 0};
      if (check_orientation) {
        float rot = A.keys[idx1].angle - B.keys[best_idx2].angle;
        if (rot < 0.0) rot += 360.0f;
        int bin = (int)std::round(rot * factor);
        if (bin == kBowHisto) bin = 0;
        if (bin < 0 || bin >= kBowHisto) {
          set_error("SearchByBoW(KF, KF): key angles outside [0, 360)");
          return VIEO_E_INVALID;
        }
        h.bin = bin, h.pos = rotHist[bin].size();
        rotHist[bin].push_back(idx1);
      }
      held.emplace(mp, h);
      nmatches++;
    }
    if (check_orientation) {
      std::vector<int> rotHist2[kBowHisto];
      for (int i = 0; i < kBowHisto; i++) {
        for (size_t j : rothist2erase[i]) rotHist[i][j] = -1;
        for (int v : rotHist[i])
          if (v != -1) rotHist2[i].push_back(v);
      }
      int ind1 = -1, ind2 = -1, ind3 = -1;
      bow_three_maxima(rotHist2, kBowHisto, ind1, ind2, ind3);
      for (int i = 0; i < kBowHisto; i++) {
        if (i == ind1 || i == ind2 || i == ind3) continue;
        for (int v : rotHist2[i]) match12[v] = -1, nmatches--;
      }
    }
    h_n_matches[p] = nmatches;
  }
  return VIEO_OK;
}
