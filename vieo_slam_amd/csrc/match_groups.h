// Host-side group tables of camm::GeometricCamera::FillMatchesFromPair (reference
// common/camera_models/camera_base.h:408-574, compiled with USE_STRATEGY_MIN_DIST: common/config.h:12) for the walk of
// SearchForTriangulation (tri_walk.h); ComputeStereoFishEyeMatches keeps the same tables on the device (k_fe_fill,
// fisheye_stereo.hip).  The bookkeeping is order dependent (a later pair can take a key from an earlier group), so it
// runs on the host in the reference's order over the candidates the device kept for every pair at once.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace vieo {

// ---- host: the group tables of FillMatchesFromPair (camera_base.h:408-574, USE_STRATEGY_MIN_DIST) ----------
struct FeGroups {
  int nc = 0;
  std::vector<int32_t> idxs;   // [g][nc], -1: none          (mvidxsMatches)
  std::vector<float> last;     // [g][nc], INFINITY: none    (lastdists)
  std::vector<uint8_t> good;   //                            (goodmatches_)
  std::vector<int32_t> key2g[8];  // (camera, key) -> group, -1: none   (mapcamidx2idxs_)
  void reset(int n_cams, const int32_t* n_keys) {
    nc = n_cams;
    idxs.clear(), last.clear(), good.clear();
    for (int c = 0; c < n_cams; ++c) key2g[c].assign(n_keys[c], -1);
  }
  int size() const { return (int)good.size(); }
};

// one accepted pair (key idxi of camera cami, key idxj of camera camj) at distance dist; false: the groups keep what they hold
static inline bool fe_fill(FeGroups& G, int cami, int idxi, int camj, int idxj, float dist) {
  const int nc = G.nc, cam[2] = {cami, camj}, key[2] = {idxi, idxj};
  int gi = G.key2g[cami][idxi];
  const int gj = G.key2g[camj][idxj];
  if (gi < 0 && gj >= 0) gi = gj;  // iteri = iterj
  if (gi < 0) {  // a new group
    const int g = G.size();
    G.idxs.insert(G.idxs.end(), nc, -1);
    G.last.insert(G.last.end(), nc, INFINITY);
    for (int t = 0; t < 2; ++t) G.idxs[(size_t)g * nc + cam[t]] = key[t], G.last[(size_t)g * nc + cam[t]] = dist, G.key2g[cam[t]][key[t]] = g;
    G.good.push_back(1);
    return true;
  }
  int g = gi, contradict = (gj >= 0 && gj != gi) ? 2 : 0;
  if (contradict) {  // keep the group whose members were matched at the smaller mean distance
    float sum[2] = {0, 0};
    int cnt[2] = {0, 0};
    for (int t = 0; t < nc; ++t) {
      if (G.idxs[(size_t)g * nc + t] >= 0) sum[0] += G.last[(size_t)g * nc + t], ++cnt[0];
      if (G.idxs[(size_t)gj * nc + t] >= 0) sum[1] += G.last[(size_t)gj * nc + t], ++cnt[1];
    }
    if (sum[1] * cnt[0] < sum[0] * cnt[1]) g = gj, contradict = 1;
  }
  int32_t* ix = &G.idxs[(size_t)g * nc];
  float* ld = &G.last[(size_t)g * nc];
  bool check[2];  // the side's key enters the group: its slot is empty, or holds another key at a larger distance
  for (int t = 0; t < 2; ++t) check[t] = ix[cam[t]] < 0 || (key[t] != ix[cam[t]] && ld[cam[t]] > dist);
  if (!(check[0] || check[1])) return false;
  if (contradict) {  // the group that lost gives up the pair's keys
    const int gc = contradict == 1 ? gi : gj;
    for (int t = 0; t < 2; ++t)
      if (key[t] == G.idxs[(size_t)gc * nc + cam[t]])
        G.key2g[cam[t]][key[t]] = -1, G.last[(size_t)gc * nc + cam[t]] = INFINITY, G.idxs[(size_t)gc * nc + cam[t]] = -1;
  }
  for (int t = 0; t < 2; ++t) {
    if (check[t] && key[t] != ix[cam[t]]) {
      if (ix[cam[t]] >= 0) G.key2g[cam[t]][ix[cam[t]]] = -1;
      if (G.key2g[cam[t]][key[t]] < 0) G.key2g[cam[t]][key[t]] = g;  // map::emplace keeps an existing entry
      ix[cam[t]] = key[t];
    }
    if (check[t] || ld[cam[t]] > dist) ld[cam[t]] = dist;
  }
  return true;
}

}  // namespace vieo
