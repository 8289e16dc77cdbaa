// The host half of the feature-vector searches (vieo_slam_amd/csrc/bow_walk.h, orb_match.h) behind a C interface, for
// tests/test_bow_walk.py: the plan of a SearchByBoW call, its distance array filled the way k_bow_distances fills it but
// with the header's host Hamming function, and the walk.  Test only.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../vieo_slam_amd/csrc/bow_walk.h"

static char g_error[512];
namespace vieo {
void set_error(const char* fmt, ...) {  // the library's keeps the text per thread; this one keeps the last
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
}
}  // namespace vieo

using namespace vieo;

// k_bow_distances on the host: descriptors of `first`, then of the n `others`; feat: the list the queries' runs point into
static std::vector<uint16_t> distances(const BowPlan& P, const vieo_bow_keys& first, const vieo_bow_keys* others, int n,
                                       const int32_t* feat) {
  std::vector<uint4> desc;  // (16 bytes per entry: two entries per key)
  auto append = [&](const vieo_bow_keys& K) {
    const size_t at = desc.size();
    desc.resize(at + 2 * (size_t)K.n_keys);
    if (K.n_keys) memcpy(&desc[at], K.descriptors, 32 * (size_t)K.n_keys);
  };
  append(first);
  for (int p = 0; p < n; p++) append(others[p]);
  std::vector<uint16_t> dist(P.n_dist + 1);
  for (const BowQuery& Q : P.queries)
    for (int k = 0; k < Q.count_f; k++)
      dist[Q.out_off + k] = (uint16_t)hamming256(&desc[2 * (size_t)Q.desc], &desc[2 * (size_t)feat[Q.first_f + k]]);
  return dist;
}

extern "C" {

const char* bw_error() { return g_error; }
int bw_constants(int which) { return which == 0 ? kThLow : which == 1 ? kThHigh : kHistoLen; }
int bw_hamming(const uint8_t* a, const uint8_t* b) {
  uint4 x[2], y[2];
  memcpy(x, a, 32), memcpy(y, b, 32);
  return hamming256(x[0], x[1], y);
}
int bw_rot_bin(float a1, float a2) { return rot_bin(a1, a2); }
unsigned bw_three_maxima(const int* counts) { return three_maxima(counts); }
int bw_node_table_ok(int n_keys, int n_nodes, const uint32_t* id, const int32_t* first, const int32_t* feat) {
  return node_table_ok(n_keys, n_nodes, id, first, feat) ? 1 : 0;
}
// the (a, b) pairs for_shared_nodes calls back with; returns their number
int bw_shared_nodes(const uint32_t* id_a, int n_a, const uint32_t* id_b, int n_b, int32_t* out) {
  int n = 0;
  for_shared_nodes(id_a, n_a, id_b, n_b, [&](int a, int b) { out[2 * n] = a, out[2 * n + 1] = b, n++; });
  return n;
}

// vieo_search_by_bow / vieo_search_by_bow_rig (key_cam null: rectified) after their checks
int bw_search_frame(const vieo_bow_keys* F, const uint8_t* key_cam, const vieo_bow_keys* kfs, int n_kfs, float nn_ratio,
                    int check_orientation, int32_t* match, int32_t* n_matches) {
  const BowPlan P = bow_plan_frame(*F, kfs, n_kfs);
  const std::vector<uint16_t> dist = distances(P, *F, kfs, n_kfs, F->node_feat);
  for (int p = 0; p < n_kfs; p++) {
    const int rc = bow_walk_frame(P, p, dist.data(), kfs[p], *F, key_cam, nn_ratio, check_orientation,
                                  match + (size_t)p * F->n_keys, n_matches + p);
    if (rc != VIEO_OK) return rc;
  }
  return VIEO_OK;
}

// vieo_search_by_bow_kf after its checks
int bw_search_kf(const vieo_bow_keys* A, const vieo_bow_keys* kf2s, int n_kf2, float nn_ratio, int check_orientation,
                 int32_t* match12, int32_t* n_matches) {
  const BowPlan P = bow_plan_kf(*A, kf2s, n_kf2);
  const std::vector<uint16_t> dist = distances(P, *A, kf2s, n_kf2, P.feat.data());
  for (int p = 0; p < n_kf2; p++) {
    const int rc = bow_walk_kf(P, p, dist.data(), *A, kf2s[p], nn_ratio, check_orientation, match12 + (size_t)p * A->n_keys,
                               n_matches + p);
    if (rc != VIEO_OK) return rc;
  }
  return VIEO_OK;
}

}  // extern "C"
