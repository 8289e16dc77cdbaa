// The host half of SearchForTriangulation and of the triangulation that follows it (vieo_slam_amd/csrc/tri_walk.h)
// behind a C interface, for tests/test_tri_walk.py: the checks, the plan, the walk over a candidate table the caller
// hands in where k_tri_gates writes one, the row gather and the result scatter.  Test only.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../vieo_slam_amd/csrc/tri_walk.h"

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

static bool any_camera(const vieo_camera&) { return true; }  // (the camera model's check stays with the device code)

static TriPlan g_plan;
static TriRows g_rows;

// FeGroups / fe_fill as they stood before their two per-side blocks became loops (with the p3d table and the tri_ok
// argument they still had), kept word for word as the yardstick of tw_fill_compare
namespace before {
struct FeGroups {
  int nc = 0;
  std::vector<int32_t> idxs;   // [g][nc], -1: none          (mvidxsMatches)
  std::vector<float> last;     // [g][nc], INFINITY: none    (lastdists)
  std::vector<uint8_t> good;   //                            (goodmatches_)
  std::vector<double> p3d;     // [g][3]                     (v3dpoints_)
  std::vector<int32_t> key2g[8];  // (camera, key) -> group, -1: none   (mapcamidx2idxs_)
  void reset(int n_cams, const int32_t* n_keys) {
    nc = n_cams;
    idxs.clear(), last.clear(), good.clear(), p3d.clear();
    for (int c = 0; c < n_cams; ++c) key2g[c].assign(n_keys[c], -1);
  }
  int size() const { return (int)good.size(); }
};

static inline bool fe_fill(FeGroups& G, int cami, int idxi, int camj, int idxj, float dist, bool tri_ok, const double* p3d) {
  const int nc = G.nc;
  int gi = G.key2g[cami][idxi];
  const int gj = G.key2g[camj][idxj];
  if (gi < 0 && gj >= 0) gi = gj;  // iteri = iterj
  int check0 = 0, check1 = 0, contradict = 0, g = -1;
  const int g_first = gi;  // iteri->second
  if (gi >= 0) {
    g = gi;
    contradict = (gj >= 0 && gj != g) ? 2 : 0;
    if (contradict) {  // keep the group whose members were matched at the smaller mean distance
      float sum[2] = {0, 0};
      int cnt[2] = {0, 0};
      for (int t = 0; t < nc; ++t) {
        if (G.idxs[(size_t)g * nc + t] >= 0) sum[0] += G.last[(size_t)g * nc + t], ++cnt[0];
        if (G.idxs[(size_t)gj * nc + t] >= 0) sum[1] += G.last[(size_t)gj * nc + t], ++cnt[1];
      }
      if (sum[1] * cnt[0] < sum[0] * cnt[1]) g = gj, contradict = 1;
    }
    const int32_t* ix = &G.idxs[(size_t)g * nc];
    const float* ld = &G.last[(size_t)g * nc];
    if (ix[cami] < 0 || (idxi != ix[cami] && ld[cami] > dist)) check0 = 2;
    if (ix[camj] < 0 || (idxj != ix[camj] && ld[camj] > dist)) check1 = 2;
  } else
    check0 = check1 = 1;
  if (!(check0 || check1)) return false;
  if (!tri_ok) return false;
  if (check0 == 1) {
    g = G.size();
    G.idxs.insert(G.idxs.end(), nc, -1);
    G.last.insert(G.last.end(), nc, INFINITY);
    G.idxs[(size_t)g * nc + cami] = idxi, G.idxs[(size_t)g * nc + camj] = idxj;
    G.last[(size_t)g * nc + cami] = dist, G.last[(size_t)g * nc + camj] = dist;
    // map::emplace keeps an existing entry; neither key has one here
    G.key2g[cami][idxi] = g, G.key2g[camj][idxj] = g;
    G.good.push_back(1);
    G.p3d.resize((size_t)G.size() * 3);
  } else {
    if (contradict) {
      const int gc = contradict == 1 ? g_first : gj;
      int32_t* ix = &G.idxs[(size_t)gc * nc];
      if (idxi == ix[cami]) G.key2g[cami][idxi] = -1, G.last[(size_t)gc * nc + cami] = INFINITY, ix[cami] = -1;
      if (idxj == ix[camj]) G.key2g[camj][idxj] = -1, G.last[(size_t)gc * nc + camj] = INFINITY, ix[camj] = -1;
    }
    int32_t* ix = &G.idxs[(size_t)g * nc];
    float* ld = &G.last[(size_t)g * nc];
    if (check0 == 2) {
      if (idxi != ix[cami]) {
        if (ix[cami] >= 0) G.key2g[cami][ix[cami]] = -1;
        if (G.key2g[cami][idxi] < 0) G.key2g[cami][idxi] = g;  // emplace
        ix[cami] = idxi;
      }
      ld[cami] = dist;
    } else if (ld[cami] > dist)
      ld[cami] = dist;
    if (check1 == 2) {
      if (idxj != ix[camj]) {
        if (ix[camj] >= 0) G.key2g[camj][ix[camj]] = -1;
        if (G.key2g[camj][idxj] < 0) G.key2g[camj][idxj] = g;
        ix[camj] = idxj;
      }
      ld[camj] = dist;
    } else if (ld[camj] > dist)
      ld[camj] = dist;
  }
  if (p3d) memcpy(&G.p3d[(size_t)g * 3], p3d, 24);
  return true;
}
}  // namespace before

extern "C" {

// n_ops pairs (ops: [n_ops][5] = cami, idxi, camj, idxj, dist; cami != camj) through fe_fill and through its earlier
// text on tables of nc cameras of n_keys keys each; after every pair the return values and the whole tables (idxs, last,
// good, key2g) must be equal.  Returns the first op after which they differ, or -1.  seen[0..3]: from the EARLIER text's
// tables before each op, how many ops met two different groups, found a slot held by another key at a larger distance
// (a displacement), opened a group, were turned away.
int tw_fill_compare(int nc, int n_keys, const int32_t* ops, int n_ops, int32_t* seen) {
  std::vector<int32_t> nk(nc, n_keys);
  FeGroups G;
  before::FeGroups B;
  G.reset(nc, nk.data()), B.reset(nc, nk.data());
  for (int k = 0; k < n_ops; k++) {
    const int32_t* o = ops + 5 * k;
    const int gi = B.key2g[o[0]][o[1]], gj = B.key2g[o[2]][o[3]];
    seen[0] += gi >= 0 && gj >= 0 && gi != gj;
    seen[2] += gi < 0 && gj < 0;
    const size_t groups = B.good.size();
    const std::vector<int32_t> idxs = B.idxs;
    const bool rb = before::fe_fill(B, o[0], o[1], o[2], o[3], (float)o[4], true, nullptr);
    const bool rg = fe_fill(G, o[0], o[1], o[2], o[3], (float)o[4]);
    seen[3] += !rb;
    for (size_t g = 0; g < groups && rb; g++)  // a slot that held a key now holds another one
      for (int c = 0; c < nc; c++) {
        const int32_t was = idxs[g * nc + c], is = B.idxs[g * nc + c];
        seen[1] += was >= 0 && is >= 0 && was != is;
      }
    bool same = rb == rg && G.idxs == B.idxs && G.good == B.good && G.last.size() == B.last.size();
    for (size_t i = 0; same && i < G.last.size(); i++) same = G.last[i] == B.last[i];  // (INFINITY == INFINITY)
    for (int c = 0; same && c < nc; c++) same = G.key2g[c] == B.key2g[c];
    if (!same) return k;
  }
  return -1;
}

const char* tw_error() { return g_error; }

// the entry's checks and the plan: st1 / st2s null = vieo_search_for_triangulation, else vieo_create_new_map_points.
// queries: [cap_q][5] as TriQuery; offs: [4][n_kf2 + 2] key, feature, level and group offsets; returns the query
// count or the error
int tw_plan(const vieo_tri_keyframe* kf1, const vieo_tri_stereo* st1, const vieo_tri_keyframe* kf2s, const vieo_tri_stereo* st2s,
            int n_kf2, int only_stereo, int32_t pair_stride, int32_t* h_pairs, int32_t* h_n_pairs, int32_t* h_n_matches,
            int8_t* h_status, double* h_x3d, float* h_x3d_f, int32_t* h_n_new, int32_t* queries, int cap_q, int32_t* q_begin,
            int32_t* offs, int64_t* n_cand) {
  TriArgs a{};
  a.search = true, a.tri = st1 != nullptr, a.kf1 = kf1, a.kf2s = kf2s, a.st1 = st1, a.st2s = st2s, a.n_kf2 = n_kf2;
  a.only_stereo = only_stereo, a.check_orientation = 1, a.pair_capacity = 1, a.pair_stride = pair_stride;
  a.h_pairs = h_pairs, a.h_n_pairs = h_n_pairs, a.h_n_matches = h_n_matches, a.rows = h_pairs, a.n_rows = h_n_pairs;
  a.h_status = h_status, a.h_x3d = h_x3d, a.h_x3d_f = h_x3d_f, a.h_n_new = h_n_new;
  std::vector<int> n_groups;
  const int rc = tri_check(a, any_camera, n_groups);
  if (rc != VIEO_OK || n_kf2 == 0) return rc;
  tri_layout(a, n_groups, g_plan);
  tri_queries(a, g_plan);
  const int nq = (int)g_plan.queries.size();
  if (nq <= cap_q && nq) memcpy(queries, g_plan.queries.data(), nq * sizeof(TriQuery));
  memcpy(q_begin, g_plan.q_begin.data(), (n_kf2 + 1) * 4);
  const std::vector<int>* o[4] = {&g_plan.key_off, &g_plan.feat_off, &g_plan.lvl_off, &g_plan.group_off};
  for (int k = 0; k < 4; k++) memcpy(offs + k * (n_kf2 + 2), o[k]->data(), (n_kf2 + 2) * 4);
  *n_cand = (int64_t)g_plan.n_cand;
  return nq;
}

// the walk of every neighbour over the plan tw_plan left; cand: [n_cand][2] (idx2, dist) at the queries' out_off
int tw_walk(const vieo_tri_keyframe* kf1, const vieo_tri_keyframe* kf2s, int n_kf2, int check_orientation, int32_t pair_capacity,
            int32_t pair_stride, const int32_t* cand, const int32_t* cand_n, int32_t* h_pairs, int32_t* h_n_pairs,
            int32_t* h_n_matches) {
  TriArgs a{};
  a.search = true, a.kf1 = kf1, a.kf2s = kf2s, a.n_kf2 = n_kf2, a.check_orientation = check_orientation;
  a.pair_capacity = pair_capacity, a.pair_stride = pair_stride;
  a.h_pairs = h_pairs, a.h_n_pairs = h_n_pairs, a.h_n_matches = h_n_matches;
  return tri_walk(a, g_plan, (const TriCand*)cand, cand_n);
}

// vieo_triangulate_new_points without its kernel: the checks and the gather; rows / row_pair / row_dst (room for every
// row of h_pairs) as the kernel gets them; returns the gathered row count or the error
int tw_gather(const vieo_tri_keyframe* kf1, const vieo_tri_stereo* st1, const vieo_tri_keyframe* kf2s, const vieo_tri_stereo* st2s,
              int n_kf2, int32_t pair_capacity, int32_t pair_stride, const int32_t* h_pairs, const int32_t* h_n_pairs, int8_t* h_status,
              double* h_x3d, float* h_x3d_f, int32_t* h_n_new, int32_t* rows, int32_t* row_pair, int64_t* row_dst) {
  TriArgs a{};
  a.tri = true, a.kf1 = kf1, a.kf2s = kf2s, a.st1 = st1, a.st2s = st2s, a.n_kf2 = n_kf2;
  a.pair_capacity = pair_capacity, a.pair_stride = pair_stride, a.rows = h_pairs, a.n_rows = h_n_pairs;
  a.h_status = h_status, a.h_x3d = h_x3d, a.h_x3d_f = h_x3d_f, a.h_n_new = h_n_new;
  std::vector<int> n_groups;
  int rc = tri_check(a, any_camera, n_groups);
  if (rc != VIEO_OK || n_kf2 == 0) return rc;
  if ((rc = tri_gather(a, g_rows)) != VIEO_OK) return rc;
  for (int r = 0; r < g_rows.n(); r++) row_pair[r] = g_rows.row_pair[r], row_dst[r] = (int64_t)g_rows.row_dst[r];
  if (g_rows.n()) memcpy(rows, g_rows.rows.data(), g_rows.rows.size() * 4);
  return g_rows.n();
}

// the scatter of the kernel's results of the rows tw_gather left
void tw_scatter(int n_kf2, int32_t pair_capacity, const int8_t* st, const double* x3d, const float* x3d_f, int8_t* h_status,
                double* h_x3d, float* h_x3d_f, int32_t* h_n_new) {
  TriArgs a{};
  a.n_kf2 = n_kf2, a.pair_capacity = pair_capacity, a.h_status = h_status, a.h_x3d = h_x3d, a.h_x3d_f = h_x3d_f, a.h_n_new = h_n_new;
  tri_scatter(a, g_rows, st, x3d, x3d_f);
}

}  // extern "C"
