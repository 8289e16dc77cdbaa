// bow_search.hip -- ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) (reference src/ORBmatcher.cc:344-505;
// Tracking::Relocalization, Tracking.cc:2554, and TrackReferenceKeyFrame, :1731) for a batch of key frames against one
// frame: vieo_search_by_bow for the rectified configuration (every key is of image 0), vieo_search_by_bow_rig for a
// rig frame (F.mapn2in_ filled: best / second best per image, the MATCH_KNN_IN_EACH_IMG branch); one walk for both,
// and ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12) (:726-905; LoopClosing::ComputeSim3) for one key frame
// against a batch of candidates (vieo_search_by_bow_kf, at the end of the file).
//   k_bow_distances  one lane per "query" = a key of a key frame that holds a map point and sits in a vocabulary node
//                    the other side shares: the Hamming distance to every key of that node there, all pairs in one
//                    launch (the pair enumeration of tri_search.hip)
//   host             bow_walk.h: the query plan, and the reference's walk over those distances, which depends on its
//                    own earlier matches.  This file keeps the checks of the arguments, the launch and the entries.
// A query's distances are as many as its node has keys on the other side, so the kernel writes without atomics.
#include <algorithm>
#include <vector>

#include "bow_walk.h"
#include "common.h"

namespace vieo {

// desc: the frame's descriptors first, then those of the key frames; feat_f: the frame's node_feat
__global__ void __launch_bounds__(64)
k_bow_distances(const BowQuery* __restrict__ queries, int n_queries, const uint8_t* __restrict__ desc,
                const int* __restrict__ feat_f, uint16_t* __restrict__ dist) {
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= n_queries) return;
  const BowQuery Q = queries[q];
  const uint8_t* d1 = desc + 32 * (size_t)Q.desc;
  for (int k = 0; k < Q.count_f; k++)
    dist[Q.out_off + k] = (uint16_t)hamming256(d1, desc + 32 * (size_t)feat_f[Q.first_f + k]);
}

static bool bow_keys_ok(const vieo_bow_keys& K, bool key_frame) {
  if (K.n_keys < 0) return false;
  if (K.n_keys > 0 && (!K.keys || !K.descriptors || (key_frame && !K.mp_id))) return false;
  for (int i = 0; i < K.n_keys; i++)  // the rotation histogram's bins (the reference asserts)
    if (!(K.keys[i].angle >= 0.f && K.keys[i].angle < 360.f)) return false;
  return node_table_ok(K.n_keys, K.n_nodes, K.node_id, K.node_first, K.node_feat);
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
  const BowPlan P = bow_plan_frame(F, kfs, n_kfs);
  std::vector<uint16_t> dist(std::max<size_t>(P.n_dist, 1));
  if ((rc = bow_run_distances(P.queries, F, kfs, n_kfs, F.node_feat, F.n_nodes ? F.node_first[F.n_nodes] : 0, dist, P.n_dist)) != VIEO_OK)
    return rc;
  for (int p = 0; p < n_kfs; p++)
    if ((rc = bow_walk_frame(P, p, dist.data(), kfs[p], F, key_cam, nn_ratio, check_orientation, h_match + (size_t)p * F.n_keys,
                             h_n_matches + p)) != VIEO_OK)
      return rc;
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
  const BowPlan P = bow_plan_kf(A, kf2s, n_kf2);
  std::vector<uint16_t> dist(std::max<size_t>(P.n_dist, 1));
  if ((rc = bow_run_distances(P.queries, A, kf2s, n_kf2, P.feat.data(), P.feat.size(), dist, P.n_dist)) != VIEO_OK) return rc;
  for (int p = 0; p < n_kf2; p++)
    if ((rc = bow_walk_kf(P, p, dist.data(), A, kf2s[p], nn_ratio, check_orientation, h_match12 + (size_t)p * A.n_keys,
                          h_n_matches + p)) != VIEO_OK)
      return rc;
  return VIEO_OK;
}
