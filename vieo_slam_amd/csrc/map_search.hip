// map_search.hip -- the map-side projection searches on gfx950: ORBmatcher::SearchByProjectionBase as local mapping's Fuse
// calls it (reference: src/ORBmatcher.cc:26-227), SearchBySim3 (:1222-1301), and the two searches of a loop closure that
// take a Sim3 world pose, SearchByProjection(KeyFrame*, Scw, ...) (:507-626) and Fuse(KeyFrame*, Scw, ...) (:1167-1220).
//
// All of them project map points into key frames and walk the window grid of sbp_grid.h, which proj_search.hip builds
// (sbp_build_grids).  The device side is one projection (fuse_project_gates) and one window walk (fuse_window_walk); the
// host side stages the key frames of a call once (KfStage) whatever the entry point.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "ba_device.h"
#include "sbp_grid.h"

namespace vieo {

// ---------------------------------------------------------------- SearchByProjectionBase (Fuse) -------------
// ORBmatcher.cc:26-193 per (map point, camera): one wavefront per point; the projection and its gates are
// evaluated by every lane (cheap, uniform), the window is walked column by column over the CSR grid with the
// lanes across a column's run, best (distance, position in the reference's candidate order) reduced over the
// wavefront.  The mutations that follow in the reference (FuseMP, only-one-match) are the caller's.
struct FuseDev {
  vieo_fuse_frame F;
  CamD cams[4];
};

// The lanes' work for one (point, camera) in two parts, shared by k_fuse_search, k_sim3_search (back to back, see
// fuse_search_lanes) and the two-launch Scw searches (k_scw_gate runs the first part one lane per item, k_scw_best /
// k_scw_list the second one wavefront per survivor).
// What the projection hands to the window walk:
struct FuseGate {
  float u, v, radius, invz;
  int lvl;
};

// Part 1 (:44-112): the projection and its gates -- the skip mask, positive depth, IsInImage, the 0.8 / 1.2 distance test,
// the viewing cone, PredictScale, the radius.  false: the (point, camera) has no window.
__device__ __forceinline__ bool fuse_project_gates(const FuseDev* __restrict__ fd, int cami, const vieo_fuse_point& P, int skip,
                                                   FuseGate* __restrict__ G) {
  const vieo_fuse_frame& FF = fd->F;
  const vieo_frustum_frame& F = FF.base;
  if ((skip & (1u << 31)) || (skip & (1 << cami))) return false;
  const float X0 = P.Xw[0], X1 = P.Xw[1], X2 = P.Xw[2];
  const float* R = F.Rcrw;
  float Pcr[3];
  for (int r = 0; r < 3; ++r) Pcr[r] = (R[r * 3] * X0 + R[r * 3 + 1] * X1 + R[r * 3 + 2] * X2) + F.tcrw[r];
  const float* Tc = F.Tcr[cami];
  float Pc[3], twc[3];
  for (int r = 0; r < 3; ++r) Pc[r] = (Tc[r * 4] * Pcr[0] + Tc[r * 4 + 1] * Pcr[1] + Tc[r * 4 + 2] * Pcr[2]) + Tc[r * 4 + 3];
  const float* t = F.trc[cami];
  for (int r = 0; r < 3; ++r) twc[r] = F.Ow[r] + (R[r] * t[0] + R[3 + r] * t[1] + R[6 + r] * t[2]);
  if (Pc[2] <= 0.0f) return false;
  const float invz = 1.0f / Pc[2];
  float u, v;
  const CamD& C = fd->cams[cami];
  if (!F.use_distort) {
    const float p0 = Pc[0] * invz, p1 = Pc[1] * invz;
    u = ((float)C.fx * p0 + 0.f * p1) + (float)C.cx * 1.f;
    v = (0.f * p0 + (float)C.fy * p1) + (float)C.cy * 1.f;
  } else {
    const double Pd[3] = {Pc[0], Pc[1], Pc[2]};
    double uv[2];
    cam_project(C, Pd, uv, nullptr);
    u = (float)uv[0], v = (float)uv[1];
  }
  const float* b = F.bounds[cami];
  if (!(u >= b[0] && u < b[1] && v >= b[2] && v < b[3])) return false;  // FrameBase::IsInImage
  const float PO[3] = {X0 - twc[0], X1 - twc[1], X2 - twc[2]};
  const float dist3D = sqrtf(PO[0] * PO[0] + PO[1] * PO[1] + PO[2] * PO[2]);
  if (dist3D < 0.8f * P.min_distance || dist3D > 1.2f * P.max_distance) return false;
  if (FF.check_viewing_angle &&
      (double)(PO[0] * P.normal[0] + PO[1] * P.normal[1] + PO[2] * P.normal[2]) < 0.5 * (double)dist3D)
    return false;
  const float ratio = P.max_distance / dist3D;
  int lvl = (int)ceilf((float)log((double)ratio) / F.log_scale_factor);  // PredictScale, see oracle/mappoint.cc
  if (lvl < 0)
    lvl = 0;
  else if (lvl >= F.n_levels)
    lvl = F.n_levels - 1;
  G->u = u, G->v = v, G->invz = invz, G->lvl = lvl;
  G->radius = FF.th_radius * FF.scale_factors[lvl];
  return true;
}

// Part 2 (:114-191): FrameBase::GetFeaturesInArea over the CSR grid, column by column with the lanes across a column's
// run, the octave and chi2 tests and the Hamming distance.  `hit(ok, dist, position in the reference's candidate order,
// key)` is called by EVERY lane once per 64 entries of a run (ok = false for a lane past the run's end or for a key that
// fails a test), so that it may vote across the wavefront; G is wave-uniform, and so is every trip count here.
template <class Hit>
__device__ __forceinline__ void fuse_window_walk(const FuseDev* __restrict__ fd, int cami, const int* __restrict__ cell_start,
                                                 const float4* __restrict__ cell_rec, const uint8_t* __restrict__ desc,
                                                 const uint8_t* __restrict__ pdesc, const FuseGate& G, int lane, Hit&& hit) {
  const vieo_fuse_frame& FF = fd->F;
  const vieo_frustum_frame& F = FF.base;
  const float* b = F.bounds[cami];
  const float u = G.u, v = G.v, radius = G.radius, invz = G.invz;
  const int lvl = G.lvl;
  const float winv = (float)kGridCols / (b[1] - b[0]), hinv = (float)kGridRows / (b[3] - b[2]);
  const int min_cellx = max(0, (int)floorf((u - b[0] - radius) * winv));
  const int max_cellx = min(kGridCols - 1, (int)ceilf((u - b[0] + radius) * winv));
  const int min_celly = max(0, (int)floorf((v - b[2] - radius) * hinv));
  const int max_celly = min(kGridRows - 1, (int)ceilf((v - b[2] + radius) * hinv));
  if (min_cellx >= kGridCols || max_cellx < 0 || min_celly >= kGridRows || max_celly < 0) return;
  const uint4 d0 = ((const uint4*)pdesc)[0], d1 = ((const uint4*)pdesc)[1];
  int order = 0;
  for (int ix = min_cellx; ix <= max_cellx; ++ix) {
    const int s0 = cell_start[ix * kGridRows + min_celly], s1 = cell_start[ix * kGridRows + max_celly + 1];
    for (int e0 = s0; e0 < s1; e0 += 64) {
      const int e = e0 + lane;
      bool ok = false;
      unsigned d = 0;
      int j = -1;
      if (e < s1) {
        const float4 k = cell_rec[e];
        const int pk = __float_as_int(k.w), oct = pk >> 16;
        j = pk & 0xFFFF;
        ok = fabsf(k.x - u) < radius && fabsf(k.y - v) < radius && oct >= lvl - 1 && oct <= lvl;
        if (ok && FF.use_bf) {
          const float ex = u - k.x, ey = v - k.y;
          if (k.z >= 0) {
            const float er = (u - F.bf * invz) - k.z;
            ok = !((double)((ex * ex + ey * ey + er * er) * FF.inv_level_sigma2[oct]) > 7.8);
          } else
            ok = !((double)((ex * ex + ey * ey) * FF.inv_level_sigma2[oct]) > 5.99);
        }
        if (ok) d = (unsigned)hamming256(d0, d1, desc + (size_t)j * 32);
      }
      hit(ok, d, order + (e - s0), j);
    }
    order += s1 - s0;
  }
}

// the walk reduced to the best (distance, position in the candidate order, key); *oi / *od are written only on a hit
__device__ __forceinline__ void fuse_window_best(const FuseDev* __restrict__ fd, int cami, const int* __restrict__ cell_start,
                                                 const float4* __restrict__ cell_rec, const uint8_t* __restrict__ desc,
                                                 const uint8_t* __restrict__ pdesc, const FuseGate& G, int lane,
                                                 int32_t* __restrict__ oi, int32_t* __restrict__ od) {
  unsigned best = 0xFFFFFFFFu;  // dist << 20 | position in the candidate order
  int bidx = -1;
  fuse_window_walk(fd, cami, cell_start, cell_rec, desc, pdesc, G, lane, [&](bool ok, unsigned d, int pos, int j) {
    if (ok) {
      const unsigned key = (d << 20) | (unsigned)min(pos, (1 << 20) - 1);
      if (key < best) best = key, bidx = j;
    }
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned e = __shfl_xor(best, o);
    const int j = __shfl_xor(bidx, o);
    if (e < best) best = e, bidx = j;
  }
  if (lane == 0 && bidx >= 0) *oi = bidx, *od = (int)(best >> 20);
}

__device__ __forceinline__ void fuse_search_lanes(const FuseDev* __restrict__ fd, int cami, const int* __restrict__ cell_start,
                                                  const float4* __restrict__ cell_rec, const uint8_t* __restrict__ desc,
                                                  const vieo_fuse_point& P, int skip, int lane, int32_t* __restrict__ oi,
                                                  int32_t* __restrict__ od) {
  if (lane == 0) *oi = -1, *od = INT_MAX;
  FuseGate G;
  if (!fuse_project_gates(fd, cami, P, skip, &G)) return;
  fuse_window_best(fd, cami, cell_start, cell_rec, desc, P.desc, G, lane, oi, od);
}

__global__ void __launch_bounds__(256)
k_fuse_search(const FuseDev* __restrict__ fd, int cami, const int* __restrict__ cell_start,
              const float4* __restrict__ cell_rec, const uint8_t* __restrict__ desc,
              const vieo_fuse_point* __restrict__ pts, int n, int32_t* __restrict__ best_idx,
              int32_t* __restrict__ best_dist) {
  const int m = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;  // wave-uniform
  if (m >= n) return;
  const int nc = fd->F.base.n_cams;
  const vieo_fuse_point& P = pts[m];
  fuse_search_lanes(fd, cami, cell_start, cell_rec, desc, P, P.skip_mask, lane, best_idx + (size_t)m * nc + cami,
                    best_dist + (size_t)m * nc + cami);
}

// ---------------------------------------------------------------- SearchBySim3 (ORBmatcher.cc:1222-1301) ----
// The two SearchByProjectionBase calls of every visit of a call: problem = (visit, direction), one wavefront per
// (problem, point, camera).  The problem's FuseDev holds the float transform of its direction and the target key
// frame's rig; all key frames stay resident side by side, slot f with its keys sorted by camera at f * key_cap, the
// grid of (f, cam) at (f * n_cams + cam) * (kGridCells + 1).
struct Sim3Problem {
  FuseDev fd;
  int src, dst;      // key-frame slots: the points are src's, the grid is dst's
  int n_points;      // src's keys
  int skip_first;    // offset of the problem's per-point masks (bit c: camera c is skipped, bit 31: no map point)
  size_t out_first;  // offset of its best_idx / best_dist [n_points][n_cams]
  int cam_k0[kMaxCams];  // first key of every camera of dst in its sorted order
};

__global__ void __launch_bounds__(256)
k_sim3_search(const Sim3Problem* __restrict__ probs, int key_cap, const int* __restrict__ cell_start,
              const float4* __restrict__ cell_rec, const uint8_t* __restrict__ desc,
              const vieo_fuse_point* __restrict__ pts, const int* __restrict__ skip, int32_t* __restrict__ best_idx,
              int32_t* __restrict__ best_dist) {
  const Sim3Problem& Q = probs[blockIdx.y];
  const int nc = Q.fd.F.base.n_cams;
  const int item = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;  // wave-uniform
  if (item >= Q.n_points * nc) return;
  const int m = item / nc, cami = item - m * nc;
  const size_t o = Q.out_first + (size_t)item;
  fuse_search_lanes(&Q.fd, cami, cell_start + (size_t)(Q.dst * nc + cami) * (kGridCells + 1),
                    cell_rec + (size_t)Q.dst * key_cap + Q.cam_k0[cami], desc + (size_t)Q.dst * key_cap * 32,
                    pts[(size_t)Q.src * key_cap + m], skip[Q.skip_first + m], lane, best_idx + o, best_dist + o);
}

// ---------------------------------------------------------------- the searches through Scw -------------------
// SearchByProjection(KeyFrame*, Scw, ...) (ORBmatcher.cc:507-626) and Fuse(KeyFrame*, Scw, ...) (:1167-1220): the problem
// is (visit, point, camera) over ONE point table shared by all visits of a call, item = (visit * n_points + point) *
// n_cams + camera.  In SearchAndFuse most loop points fall outside most key frames, so the gates run one lane per item
// (k_scw_gate) and only the survivors get a wavefront for their window (k_scw_best / k_scw_list).  The order of the
// survivors differs from run to run; every output is addressed by item.
struct ScwVisitDev {
  FuseDev fd;            // the float transform of the visit's Scw and the target key frame's rig
  int dst;               // the key-frame slot
  int cam_k0[kMaxCams];  // first key of every camera of dst in its sorted order
};
struct ScwSurvivor {
  int item;
  float u, v;
  int lvl;
  float radius, invz;
};
struct ScwCand {
  int key, dist, order;  // key: position in dst's camera-sorted order; order: position in the reference's candidate order
};

// one lane per item: the gates; out_a / out_b [n_items] get the value that stands for "nothing" (best: -1 / INT_MAX,
// list: first 0 / count 0); the survivors are compacted with a ballot and one atomic per wavefront
__global__ void __launch_bounds__(256)
k_scw_gate(const ScwVisitDev* __restrict__ visits, int n_items, int n_points, int nc, const vieo_fuse_point* __restrict__ pts,
           const int* __restrict__ skip, ScwSurvivor* __restrict__ surv, int* __restrict__ n_surv, int32_t* __restrict__ out_a,
           int32_t init_a, int32_t* __restrict__ out_b, int32_t init_b) {
  const int item = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  bool pass = false;
  FuseGate G;
  if (item < n_items) {
    const int vm = item / nc, c = item - vm * nc, v = vm / n_points, m = vm - v * n_points;
    out_a[item] = init_a, out_b[item] = init_b;
    pass = fuse_project_gates(&visits[v].fd, c, pts[m], skip[vm], &G);
  }
  const unsigned long long bal = __ballot(pass);
  if (!bal) return;  // (wave-uniform)
  int base = 0;
  if (lane == 0) base = atomicAdd(n_surv, __popcll(bal));
  base = __shfl(base, 0);
  if (pass) {
    ScwSurvivor S;
    S.item = item, S.u = G.u, S.v = G.v, S.lvl = G.lvl, S.radius = G.radius, S.invz = G.invz;
    surv[base + __popcll(bal & ((1ull << lane) - 1ull))] = S;  // (base + rank < n_items: at most one record per item)
  }
}

// the window of survivor s: everything wave-uniform
struct ScwWindow {
  const FuseDev* fd;
  const int* cell_start;
  const float4* cell_rec;
  const uint8_t *desc, *pdesc;
  int item, cami;
  FuseGate G;
};
__device__ __forceinline__ ScwWindow scw_window(const ScwVisitDev* __restrict__ visits, const ScwSurvivor& S, int n_points, int nc,
                                                int key_cap, const int* __restrict__ cell_start,
                                                const float4* __restrict__ cell_rec, const uint8_t* __restrict__ desc,
                                                const vieo_fuse_point* __restrict__ pts) {
  ScwWindow W;
  const int vm = S.item / nc, c = S.item - vm * nc, v = vm / n_points, m = vm - v * n_points;
  const ScwVisitDev& Q = visits[v];
  W.fd = &Q.fd, W.item = S.item, W.cami = c;
  W.cell_start = cell_start + (size_t)(Q.dst * nc + c) * (kGridCells + 1);
  W.cell_rec = cell_rec + (size_t)Q.dst * key_cap + Q.cam_k0[c];
  W.desc = desc + (size_t)Q.dst * key_cap * 32, W.pdesc = pts[m].desc;
  W.G.u = S.u, W.G.v = S.v, W.G.radius = S.radius, W.G.invz = S.invz, W.G.lvl = S.lvl;
  return W;
}

// one wavefront per survivor (the wavefronts of the grid stride over them): the best key, as fuse_search_lanes
__global__ void __launch_bounds__(256)
k_scw_best(const ScwVisitDev* __restrict__ visits, int n_points, int nc, int key_cap, const int* __restrict__ cell_start,
           const float4* __restrict__ cell_rec, const uint8_t* __restrict__ desc, const vieo_fuse_point* __restrict__ pts,
           const ScwSurvivor* __restrict__ surv, const int* __restrict__ n_surv, int32_t* __restrict__ best_idx,
           int32_t* __restrict__ best_dist) {
  const int lane = threadIdx.x & 63, n_waves = gridDim.x * 4, n = *n_surv;
  for (int s = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); s < n; s += n_waves) {
    const ScwWindow W = scw_window(visits, surv[s], n_points, nc, key_cap, cell_start, cell_rec, desc, pts);
    fuse_window_best(W.fd, W.cami, W.cell_start, W.cell_rec, W.desc, W.pdesc, W.G, lane, best_idx + W.item, best_dist + W.item);
  }
}

// one wavefront per survivor: EVERY window candidate with Hamming distance <= TH_LOW, in the reference's candidate order.
// The window is walked twice: the first walk counts, one atomic on *cursor reserves exactly that many entries of the
// pool, the second walk fills them (rank inside a run by ballot, so the entries of an item ascend in `order`).
// A reservation past pool_cap writes nothing: the host reads *cursor = the exact total, makes the pool that large and
// launches this kernel again, so no list is ever cut.
__global__ void __launch_bounds__(256)
k_scw_list(const ScwVisitDev* __restrict__ visits, int n_points, int nc, int key_cap, const int* __restrict__ cell_start,
           const float4* __restrict__ cell_rec, const uint8_t* __restrict__ desc, const vieo_fuse_point* __restrict__ pts,
           const ScwSurvivor* __restrict__ surv, const int* __restrict__ n_surv, int32_t* __restrict__ list_first,
           int32_t* __restrict__ list_count, ScwCand* __restrict__ pool, int pool_cap, int* __restrict__ cursor) {
  const int lane = threadIdx.x & 63, n_waves = gridDim.x * 4, n = *n_surv;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int s = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); s < n; s += n_waves) {
    const ScwWindow W = scw_window(visits, surv[s], n_points, nc, key_cap, cell_start, cell_rec, desc, pts);
    int cnt = 0;
    fuse_window_walk(W.fd, W.cami, W.cell_start, W.cell_rec, W.desc, W.pdesc, W.G, lane,
                     [&](bool ok, unsigned d, int, int) { cnt += __popcll(__ballot(ok && d <= (unsigned)kThLow)); });
    if (cnt == 0) continue;
    int first = 0;
    // the cursor saturates at INT_MAX instead of wrapping: past 2^31 listed candidates every later reservation is refused
    // here and the host sees a total beyond its limit
    if (lane == 0) {
      first = atomicAdd(cursor, cnt);
      if (first < 0 || first > INT_MAX - cnt) atomicExch(cursor, INT_MAX), first = INT_MAX;
    }
    first = __shfl(first, 0);
    if (lane == 0) list_first[W.item] = first, list_count[W.item] = cnt;
    if (first > pool_cap - cnt) continue;  // (pool_cap >= cnt or the subtraction is negative: no wrap either way)
    int w = first;
    fuse_window_walk(W.fd, W.cami, W.cell_start, W.cell_rec, W.desc, W.pdesc, W.G, lane, [&](bool ok, unsigned d, int pos, int j) {
      const bool h = ok && d <= (unsigned)kThLow;
      const unsigned long long bal = __ballot(h);
      if (h) {
        ScwCand c;
        c.key = j, c.dist = (int)d, c.order = pos;
        pool[w + __popcll(bal & below)] = c;
      }
      w += __popcll(bal);
    });
  }
}

}  // namespace vieo

using namespace vieo;

// ---------------------------------------------------------------- the key frames of a call: host -------------
namespace {

// a key frame of the call as the host walks read it
struct LoopKfHost {
  const vieo_loop_keyframe* K = nullptr;
  int n = 0;
  std::vector<int> perm;                      // camera-sorted position -> key
  int k0[kMaxCams + 1] = {};                  // first sorted position of every camera
  std::vector<std::pair<int, int>> by_id;     // (mp_id, key) ascending: GetIndexInKeyFrame
  CamD cams[kMaxCams];
  int cam(int i) const { return K->cam_of_key ? K->cam_of_key[i] : 0; }
  // the keys that hold map point `id`, ascending
  std::pair<const std::pair<int, int>*, const std::pair<int, int>*> keys_of(int id) const {
    auto lo = std::lower_bound(by_id.begin(), by_id.end(), std::make_pair(id, INT_MIN));
    auto hi = std::upper_bound(by_id.begin(), by_id.end(), std::make_pair(id, INT_MAX));
    return {by_id.data() + (lo - by_id.begin()), by_id.data() + (hi - by_id.begin())};
  }
};

int loop_kf_prepare(const vieo_loop_keyframe* K, const vieo_loop_keyframe* first, const char* who, int slot, LoopKfHost& H) {
  const int n = K->bow.n_keys;
  if (n < 0 || (n > 0 && (!K->bow.keys || !K->bow.descriptors || !K->bow.mp_id || !K->points)) || !K->cams) {
    set_error("%s: key frame %d has a null pointer or a negative key count", who, slot);
    return VIEO_E_INVALID;
  }
  if (n > kMaxKeys) {
    set_error("%s: key frame %d has %d keys (limit %d)", who, slot, n, kMaxKeys);
    return VIEO_E_CAPACITY;
  }
  if (K->n_cams < 1 || K->n_cams > kMaxCams || K->n_levels < 1 || K->n_levels > 16) {
    set_error("%s: key frame %d has n_cams = %d (1..4), n_levels = %d (1..16)", who, slot, K->n_cams, K->n_levels);
    return VIEO_E_INVALID;
  }
  if (K->n_cams != first->n_cams || memcmp(K->bounds, first->bounds, sizeof(float) * 4 * K->n_cams) != 0) {
    set_error("%s: key frame %d differs from the current key frame in n_cams or in the image bounds", who, slot);
    return VIEO_E_INVALID;
  }
  for (int c = 0; c < K->n_cams; ++c)
    if (!cam_from_abi(K->cams[c], H.cams[c])) {
      set_error("%s: camera %d of key frame %d has an unknown model or coefficient count", who, c, slot);
      return VIEO_E_INVALID;
    }
  H.K = K, H.n = n;
  int cnt[kMaxCams + 1] = {};
  for (int i = 0; i < n; ++i) {
    const int c = H.cam(i), o = K->bow.keys[i].octave;
    if (c < 0 || c >= K->n_cams || o < 0 || o >= K->n_levels) {
      set_error("%s: key %d of key frame %d has camera %d (of %d) / octave %d (of %d)", who, i, slot, c, K->n_cams, o, K->n_levels);
      return VIEO_E_INVALID;
    }
    cnt[c + 1]++;
  }
  for (int c = 0; c < kMaxCams; ++c) cnt[c + 1] += cnt[c];
  for (int c = 0; c <= kMaxCams; ++c) H.k0[c] = cnt[c];
  H.perm.resize(n);
  H.by_id.clear();
  for (int i = 0; i < n; ++i) {
    H.perm[cnt[H.cam(i)]++] = i;
    if (K->bow.mp_id[i] >= 0) H.by_id.emplace_back(K->bow.mp_id[i], i);
  }
  std::sort(H.by_id.begin(), H.by_id.end());
  return VIEO_OK;
}

// The key frames of one map-side call on the device, staged the same way whatever the entry point.  Slot f holds key_cap
// key positions, the keys of its cameras in consecutive ranges of them (cam_first).  Keys and descriptors are written in
// that order straight into the pinned block, which goes up in ONE copy together with what the caller adds through `s`
// (through pageable memory a 512 000-item call took three times as long); then uright is filled and the
// grids are built.  A call is open() -- the layout of the key frames, every size and offset computed anew --, the caller's
// own s.in / s.out / s.scratch in that order, upload(), the launches, s.download() and key() on what comes back.
struct KfStage {
  Staging s;
  DevBuf pool;         // a result whose size the device decides (the candidate lists of the Scw search) ...
  PinnedBuf pool_pin;  // ... and where it lands on the host
  int n_slots = 0, nc = 0, key_cap = 0;
  int k0[kMaxCams + 1] = {};  // (per-camera arrays) the first position of every camera

  // prepared key frames; with_points: their map points in KEY order beside them (zero where a key holds none)
  void open(const std::vector<LoopKfHost>& kfs, bool with_points) {
    H = kfs.data(), n_slots = (int)kfs.size(), nc = kfs[0].K->n_cams, key_cap = 1;
    for (const LoopKfHost& h : kfs) key_cap = std::max(key_cap, h.n);
    layout(kfs[0].K->bounds, with_points, false);
  }
  // one frame's per-camera arrays as the cam_first ranges of ONE slot; uright[c] == nullptr: camera c is monocular
  void open(const vieo_frustum_frame& F, const vieo_keypoint* const* keys, const float* const* uright, const uint8_t* const* desc,
            const int32_t* n_keys) {
    H = nullptr, n_slots = 1, nc = F.n_cams, cam_keys = keys, cam_ur = uright, cam_desc = desc;
    for (int c = 0; c < nc; ++c) k0[c + 1] = k0[c] + n_keys[c];  // (k0[0] stays 0)
    key_cap = std::max(1, k0[nc]);
    layout(F.bounds, false, uright != nullptr);
  }
  int upload(hipStream_t st) {
    const size_t n = (size_t)n_slots * key_cap;
    if (!ur_in) o_ur = s.scratch(n * 4);
    const size_t o_cursor = s.scratch((size_t)n_slots * 4);
    o_start = s.scratch((size_t)n_slots * nc * (kGridCells + 1) * 4), o_rec = s.scratch(n * sizeof(float4)), o_ang = s.scratch(n * 4);
    int rc;
    if ((rc = s.alloc()) != VIEO_OK) return rc;
    H ? write_key_frames() : write_cameras();
    if ((rc = s.upload(st)) != VIEO_OK) return rc;
    // no uright from the caller: a negative float in every key, all of them monocular
    if (!ur_in) VIEO_HIP_CHECK(hipMemsetAsync(s.d<float>(o_ur), 0xBF, n * 4, st));
    in.keys = s.d<vieo_keypoint>(o_keys), in.uright = s.d<float>(o_ur), in.cam_first = s.d<int>(o_cam_first), in.cursor = s.d<int>(o_cursor);
    return sbp_build_grids(in, n_slots, grid(), st);
  }
  SbpGrid grid() const { return SbpGrid{s.d<int>(o_start), s.d<float4>(o_rec), s.d<float>(o_ang), key_cap, nc}; }
  const uint8_t* desc() const { return s.d<uint8_t>(o_desc); }                   // [slot][key_cap][32] in position order
  const vieo_fuse_point* points() const { return s.d<vieo_fuse_point>(o_pts); }  // [slot][key_cap] in key order
  // a position of slot f, as the grid's records carry it, back as the caller's index: the key of a prepared key frame, or
  // the index into camera c's array.  Valid while the caller's key frames are.
  int key(int f, int c, int pos) const { return H ? H[f].perm[pos] : pos - k0[c]; }

 private:
  void layout(const float (*bounds)[4], bool points, bool uright) {
    s.reset();
    memset(in.bounds, 0, sizeof(in.bounds));
    memcpy(in.bounds, bounds, sizeof(float) * 4 * nc);
    const size_t n = (size_t)n_slots * key_cap;
    o_keys = s.in(nullptr, n * sizeof(vieo_keypoint)), o_desc = s.in(nullptr, n * 32);
    o_cam_first = s.in(nullptr, (size_t)n_slots * (nc + 1) * 4);
    with_points = points, ur_in = uright;
    o_pts = with_points ? s.in(nullptr, n * sizeof(vieo_fuse_point)) : 0;
    o_ur = ur_in ? s.in(nullptr, n * 4) : 0;
  }
  void write_key_frames() {
    for (int f = 0; f < n_slots; ++f) {
      const LoopKfHost& h = H[f];
      const size_t at = (size_t)f * key_cap;
      for (int p = 0; p < h.n; ++p) {
        s.hw<vieo_keypoint>(o_keys)[at + p] = h.K->bow.keys[h.perm[p]];
        memcpy(s.hw<uint8_t>(o_desc) + (at + p) * 32, h.K->bow.descriptors + (size_t)h.perm[p] * 32, 32);
      }
      memcpy(s.hw<int>(o_cam_first) + (size_t)f * (nc + 1), h.k0, (size_t)(nc + 1) * 4);
      for (int i = 0; i < (with_points ? h.n : 0); ++i)
        s.hw<vieo_fuse_point>(o_pts)[at + i] = h.K->bow.mp_id[i] >= 0 ? h.K->points[i] : vieo_fuse_point{};
    }
  }
  void write_cameras() {
    for (int c = 0; c < nc; ++c) {
      const int nk = k0[c + 1] - k0[c];
      if (nk == 0) continue;
      memcpy(s.hw<vieo_keypoint>(o_keys) + k0[c], cam_keys[c], (size_t)nk * sizeof(vieo_keypoint));
      memcpy(s.hw<uint8_t>(o_desc) + (size_t)k0[c] * 32, cam_desc[c], (size_t)nk * 32);
      if (ur_in && cam_ur[c])
        memcpy(s.hw<float>(o_ur) + k0[c], cam_ur[c], (size_t)nk * 4);
      else if (ur_in)
        std::fill_n(s.hw<float>(o_ur) + k0[c], nk, -1.f);
    }
    memcpy(s.hw<int>(o_cam_first), k0, (size_t)(nc + 1) * 4);
  }
  const LoopKfHost* H = nullptr;  // the source of the slots: prepared key frames, or per-camera arrays
  const vieo_keypoint* const* cam_keys = nullptr;
  const float* const* cam_ur = nullptr;
  const uint8_t* const* cam_desc = nullptr;
  SbpGridKeys in = {};
  bool with_points = false, ur_in = false;
  size_t o_keys = 0, o_desc = 0, o_cam_first = 0, o_pts = 0, o_ur = 0, o_start = 0, o_rec = 0, o_ang = 0;
};
thread_local KfStage g_kf;

}  // namespace

extern "C" {

int vieo_fuse_search(const vieo_fuse_frame* h_frame, const vieo_keypoint* const* h_keys,
                     const float* const* h_uright, const uint8_t* const* h_desc, const int32_t* n_keys,
                     const vieo_fuse_point* h_points, int n_points, int32_t* h_best_idx, int32_t* h_best_dist) {
  if (!h_frame || !h_keys || !h_desc || !n_keys || n_points < 0 || (n_points > 0 && (!h_points || !h_best_idx || !h_best_dist)))
    return VIEO_E_INVALID;
  const vieo_frustum_frame& F = h_frame->base;
  const int nc = F.n_cams;
  if (nc < 1 || nc > 4 || !F.cams || F.n_levels <= 0 || F.n_levels > 16) {
    set_error("SearchByProjectionBase: n_cams = %d (1..4) with cameras, n_levels = %d (1..16)", nc, F.n_levels);
    return VIEO_E_INVALID;
  }
  int rc = require_device();
  if (rc != VIEO_OK) return rc;
  if (n_points == 0) return VIEO_OK;
  FuseDev fd;
  memset(&fd, 0, sizeof(fd));
  fd.F = *h_frame;
  fd.F.base.cams = nullptr;
  for (int c = 0; c < nc; ++c) {
    if (!cam_from_abi(F.cams[c], fd.cams[c])) {
      set_error("SearchByProjectionBase: camera %d has an unknown model or coefficient count", c);
      return VIEO_E_INVALID;
    }
    if (n_keys[c] < 0 || n_keys[c] > kMaxKeys || (n_keys[c] > 0 && (!h_keys[c] || !h_desc[c]))) {
      set_error("SearchByProjectionBase: camera %d has %d keys (limit %d)", c, n_keys[c], kMaxKeys);
      return n_keys[c] > kMaxKeys ? VIEO_E_CAPACITY : VIEO_E_INVALID;
    }
  }
  // the cameras side by side in one slot: one upload, the grids of all cameras in one launch, a search per camera with
  // nothing in between, one download
  KfStage& K = g_kf;
  K.open(F, h_keys, h_uright, h_desc, n_keys);
  const size_t n_out = (size_t)n_points * nc;
  const size_t o_fd = K.s.in(&fd, sizeof(fd)), o_pts = K.s.in(h_points, (size_t)n_points * sizeof(vieo_fuse_point));
  const size_t o_idx = K.s.out(n_out * 4), o_dist = K.s.out(n_out * 4);
  if ((rc = K.upload(0)) != VIEO_OK) return rc;
  const SbpGrid G = K.grid();
  for (int c = 0; c < nc; ++c)
    hipLaunchKernelGGL(k_fuse_search, dim3((n_points + 3) / 4), dim3(256), 0, 0, K.s.d<FuseDev>(o_fd), c,
                       G.cell_start + c * (kGridCells + 1), G.cell_rec + K.k0[c], K.desc(), K.s.d<vieo_fuse_point>(o_pts), n_points, K.s.d<int32_t>(o_idx),
                       K.s.d<int32_t>(o_dist));
  VIEO_HIP_CHECK(hipGetLastError());
  if ((rc = K.s.download(o_idx, 0)) != VIEO_OK) return rc;
  const int32_t* bi = (const int32_t*)K.s.h(o_idx);
  for (size_t e = 0; e < n_out; ++e) h_best_idx[e] = bi[e] >= 0 ? K.key(0, (int)(e % nc), bi[e]) : bi[e];
  memcpy(h_best_dist, K.s.h(o_dist), n_out * 4);
  return VIEO_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- vieo_search_by_sim3: host -----------------
namespace {

// C = A * B (3 x 3, float, row times column summed left to right), y = A * x
inline void mat3_mul(const float* A, const float* B, float* C) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) C[r * 3 + c] = (A[r * 3] * B[c] + A[r * 3 + 1] * B[3 + c]) + A[r * 3 + 2] * B[6 + c];
}
inline void mat3_vec(const float* A, const float* x, float* y) {
  for (int r = 0; r < 3; ++r) y[r] = (A[r * 3] * x[0] + A[r * 3 + 1] * x[1]) + A[r * 3 + 2] * x[2];
}

// the FuseDev of one direction: `dst`'s rig and pyramid, the transform world -> dst's rig frame through the Sim3
void sim3_fuse_dev(const LoopKfHost& dst, const float* Rcrw, const float* tcrw, float th, FuseDev& fd) {
  memset(&fd, 0, sizeof(fd));
  const vieo_loop_keyframe& K = *dst.K;
  vieo_frustum_frame& F = fd.F.base;
  memcpy(F.Rcrw, Rcrw, sizeof(F.Rcrw)), memcpy(F.tcrw, tcrw, sizeof(F.tcrw)), memcpy(F.Ow, K.Ow, sizeof(F.Ow));
  F.n_cams = K.n_cams, F.use_distort = K.use_distort, F.cams = nullptr;
  memcpy(F.Tcr, K.Tcr, sizeof(F.Tcr)), memcpy(F.trc, K.trc, sizeof(F.trc)), memcpy(F.bounds, K.bounds, sizeof(F.bounds));
  F.log_scale_factor = K.log_scale_factor, F.n_levels = K.n_levels;
  memcpy(fd.F.scale_factors, K.scale_factors, sizeof(K.scale_factors));
  memcpy(fd.F.inv_level_sigma2, K.inv_level_sigma2, sizeof(K.inv_level_sigma2));
  fd.F.th_radius = th;  // bCheckViewingAngle = false, pbf = nullptr
  for (int c = 0; c < K.n_cams; ++c) fd.cams[c] = dst.cams[c];
}

const int kSim3MaxVisits = 16384;  // two problems per visit on the grid's y axis

struct Sim3Tap {
  bool valid = false;
  int n_visits = 0, nc = 0;
  std::vector<size_t> first;   // [visit][2]
  std::vector<int> n_points;   // [visit][2]
  std::vector<int32_t> idx, dist;  // best_idx as keys of the target key frame
};
thread_local Sim3Tap g_sim3_tap;

}  // namespace

extern "C" {

int vieo_search_by_sim3(const vieo_loop_keyframe* kf1, const vieo_loop_keyframe* kf2s, int n_kf2, vieo_sim3_visit* visits,
                        int n_visits, float th) {
  static const char* who = "SearchBySim3";
  if (!kf1 || !kf2s || n_kf2 <= 0 || n_visits < 0 || (n_visits > 0 && !visits) || !(th > 0.f)) {
    set_error("%s: a null pointer, no candidate, a negative visit count or th <= 0", who);
    return VIEO_E_INVALID;
  }
  if (n_visits > kSim3MaxVisits) {
    set_error("%s: %d visits in one call (limit %d)", who, n_visits, kSim3MaxVisits);
    return VIEO_E_CAPACITY;
  }
  const int n_slots = 1 + n_kf2;
  std::vector<LoopKfHost> H(n_slots);
  int rc;
  for (int f = 0; f < n_slots; ++f)
    if ((rc = loop_kf_prepare(f ? kf2s + (f - 1) : kf1, kf1, who, f, H[f])) != VIEO_OK) return rc;
  const int nc = kf1->n_cams, N1 = H[0].n;
  for (int v = 0; v < n_visits; ++v) {
    const vieo_sim3_visit& V = visits[v];
    if (V.kf2 < 0 || V.kf2 >= n_kf2 || (N1 > 0 && !V.match12) || !(V.s12 > 0.f)) {
      set_error("%s: visit %d names candidate %d (of %d), has no match12 or s12 <= 0", who, v, V.kf2, n_kf2);
      return VIEO_E_INVALID;
    }
    const int N2 = H[1 + V.kf2].n;
    for (int i = 0; i < N1; ++i)
      if (V.match12[i] < -1 || V.match12[i] >= N2) {
        set_error("%s: match12[%d] = %d of visit %d is outside the candidate's %d keys", who, i, V.match12[i], v, N2);
        return VIEO_E_INVALID;
      }
  }
  if ((rc = require_device()) != VIEO_OK) return rc;
  g_sim3_tap.valid = false;
  if (n_visits == 0) return VIEO_OK;

  // ---- the problems: (visit, direction)
  const int n_probs = 2 * n_visits;
  std::vector<Sim3Problem> probs(n_probs);
  std::vector<int> skip;
  size_t out_total = 0;
  int max_items = 0;
  for (int v = 0; v < n_visits; ++v) {
    const vieo_sim3_visit& V = visits[v];
    const LoopKfHost &h1 = H[0], &h2 = H[1 + V.kf2];
    const vieo_loop_keyframe &K1 = *h1.K, &K2 = *h2.K;
    float sR12[9], sR21[9], t21[3], Rt[9], R[9], t[3];
    const float inv_s = (float)(1.0 / (double)V.s12);
    for (int i = 0; i < 9; ++i) sR12[i] = V.s12 * V.R12[i];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) Rt[r * 3 + c] = V.R12[c * 3 + r];
    for (int i = 0; i < 9; ++i) sR21[i] = inv_s * Rt[i];
    mat3_vec(sR21, V.t12, t21);
    for (int r = 0; r < 3; ++r) t21[r] = -t21[r];
    for (int dir = 0; dir < 2; ++dir) {
      Sim3Problem& Q = probs[2 * v + dir];
      const LoopKfHost &src = dir ? h2 : h1, &dst = dir ? h1 : h2;
      if (!dir) {  // sR21 * R1w, sR21 * t1w + t21
        mat3_mul(sR21, K1.Rcw, R), mat3_vec(sR21, K1.tcw, t);
        for (int r = 0; r < 3; ++r) t[r] += t21[r];
      } else {  // sR12 * R2w, sR12 * t2w + t12
        mat3_mul(sR12, K2.Rcw, R), mat3_vec(sR12, K2.tcw, t);
        for (int r = 0; r < 3; ++r) t[r] += V.t12[r];
      }
      sim3_fuse_dev(dst, R, t, th, Q.fd);
      Q.src = dir ? 1 + V.kf2 : 0, Q.dst = dir ? 0 : 1 + V.kf2;
      Q.n_points = src.n, Q.skip_first = (int)skip.size(), Q.out_first = out_total;
      for (int c = 0; c < kMaxCams; ++c) Q.cam_k0[c] = dst.k0[c];
      skip.resize(skip.size() + src.n);
      int* sk = skip.data() + Q.skip_first;
      for (int i = 0; i < src.n; ++i) sk[i] = src.K->bow.mp_id[i] >= 0 ? 0 : INT_MIN;
      out_total += (size_t)src.n * nc;
      max_items = std::max(max_items, src.n * nc);
    }
    // vbAlreadyMatched1 / 2 (:1246-1261)
    int *sk1 = skip.data() + probs[2 * v].skip_first, *sk2 = skip.data() + probs[2 * v + 1].skip_first;
    for (int i = 0; i < N1; ++i) {
      const int idx2 = V.match12[i];
      if (idx2 < 0 || K2.bow.mp_id[idx2] < 0) continue;
      sk1[i] |= 1 << h1.cam(i);
      const auto range = h2.keys_of(K2.bow.mp_id[idx2]);
      for (auto it = range.first; it != range.second; ++it) sk2[it->second] |= 1 << h2.cam(it->second);
    }
  }
  if (out_total == 0 || max_items == 0) {
    for (int v = 0; v < n_visits; ++v) visits[v].n_found = 0;
    return VIEO_OK;
  }

  // ---- the key frames side by side with their points, the grids, one launch over every problem
  KfStage& K = g_kf;
  K.open(H, true);
  const size_t o_prob = K.s.in(probs.data(), probs.size() * sizeof(Sim3Problem)), o_skip = K.s.in(skip.data(), skip.size() * 4);
  const size_t o_out = K.s.out(2 * out_total * 4);  // best_idx, then best_dist
  if ((rc = K.upload(0)) != VIEO_OK) return rc;
  const SbpGrid G = K.grid();
  int32_t *d_idx = K.s.d<int32_t>(o_out), *d_dist = d_idx + out_total;
  hipLaunchKernelGGL(k_sim3_search, dim3((max_items + 3) / 4, n_probs), dim3(256), 0, 0, K.s.d<Sim3Problem>(o_prob), K.key_cap,
                     G.cell_start, G.cell_rec, K.desc(), K.points(), K.s.d<int>(o_skip), d_idx, d_dist);
  VIEO_HIP_CHECK(hipGetLastError());
  if ((rc = K.s.download(o_out, 0)) != VIEO_OK) return rc;
  Sim3Tap& T = g_sim3_tap;
  const int32_t* h_out = (const int32_t*)K.s.h(o_out);
  T.idx.assign(h_out, h_out + out_total), T.dist.assign(h_out + out_total, h_out + 2 * out_total);
  T.n_visits = n_visits, T.nc = nc;
  T.first.resize(n_probs), T.n_points.resize(n_probs);
  for (int q = 0; q < n_probs; ++q) {
    T.first[q] = probs[q].out_first, T.n_points[q] = probs[q].n_points;
    int32_t* bi = T.idx.data() + probs[q].out_first;
    for (size_t e = 0; e < (size_t)probs[q].n_points * nc; ++e)
      if (bi[e] >= 0) bi[e] = K.key(probs[q].dst, (int)(e % nc), bi[e]);  // position in the camera order -> key
  }
  T.valid = true;

  // ---- the order-dependent rest (:193-225, :1282-1298)
  std::vector<int> vn[2];  // per point the map point whose keys vnMatch holds, -1: empty
  for (int v = 0; v < n_visits; ++v) {
    vieo_sim3_visit& V = visits[v];
    const LoopKfHost &h1 = H[0], &h2 = H[1 + V.kf2];
    for (int dir = 0; dir < 2; ++dir) {
      const Sim3Problem& Q = probs[2 * v + dir];
      const LoopKfHost &src = dir ? h2 : h1, &dst = dir ? h1 : h2;
      const int32_t *bi = T.idx.data() + Q.out_first, *bd = T.dist.data() + Q.out_first;
      vn[dir].assign(src.n, -1);
      for (int i = 0; i < src.n; ++i) {
        if (src.K->bow.mp_id[i] < 0) continue;
        int best_dist = INT_MAX, best_idx = -1;
        for (int c = 0; c < nc; ++c) {
          const int d = bd[(size_t)i * nc + c], k = bi[(size_t)i * nc + c];
          if (k >= 0 && d < best_dist && dst.K->bow.mp_id[k] >= 0) best_dist = d, best_idx = k;
        }
        if (best_dist <= kThHigh) vn[dir][i] = dst.K->bow.mp_id[best_idx];
      }
    }
    int n_found = 0;
    for (int i1 = 0; i1 < N1; ++i1) {
      if (vn[0][i1] < 0) continue;
      const auto range = h2.keys_of(vn[0][i1]);
      for (auto it = range.first; it != range.second; ++it) {
        const int idx2 = it->second;
        if (vn[1][idx2] >= 0 && vn[1][idx2] == h1.K->bow.mp_id[i1]) {
          V.match12[i1] = idx2;
          n_found++;
          break;
        }
      }
    }
    V.n_found = n_found;
  }
  return VIEO_OK;
}

int vieo_search_by_sim3_tap(int visit, int direction, int32_t* best_idx, int32_t* best_dist) {
  const Sim3Tap& T = g_sim3_tap;
  if (!T.valid) return VIEO_E_EMPTY;
  if (visit < 0 || visit >= T.n_visits || direction < 0 || direction > 1) return VIEO_E_INVALID;
  const int q = 2 * visit + direction;
  const size_t n = (size_t)T.n_points[q] * T.nc;
  if (best_idx && n) memcpy(best_idx, T.idx.data() + T.first[q], n * 4);
  if (best_dist && n) memcpy(best_dist, T.dist.data() + T.first[q], n * 4);
  return VIEO_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- the searches through Scw: host ------------
namespace {

const int kScwMaxVisits = 16384;
const long long kScwMaxPointVisits = 1ll << 20;  // survivor records: 24 bytes x n_points x n_visits x n_cams at most
const long long kScwMaxListed = 1ll << 27;       // entries of the candidate pool (12 bytes each)

struct ScwTap {
  bool valid = false;
  int n_visits = 0, n_points = 0, nc = 0;
  std::vector<int32_t> a, b;    // [item]: list form first / count, best form best_idx / best_dist
  std::vector<ScwCand> pool;    // list form; key = the key frame's key
};
thread_local ScwTap g_scw_list_tap, g_scw_best_tap;
thread_local struct {
  bool valid = false;
  long long items = 0, survivors = 0;
} g_scw_stats;

struct ScwCall {
  std::vector<LoopKfHost> H;
  std::vector<ScwVisitDev> vis;
  std::vector<int> skip;  // [visit][point]: bit c = camera c is skipped, bit 31 = the point is not searched
  int nc = 0, n_points = 0, n_visits = 0;
};

// everything that refuses a call, before anything is written or launched
template <class Visit>
int scw_check(const char* who, const vieo_loop_keyframe* kfs, int n_kf, const vieo_fuse_point* points, const int32_t* point_id,
              int n_points, const Visit* visits, int n_visits, float th, ScwCall& C) {
  if (!kfs || n_kf <= 0 || n_points < 0 || (n_points > 0 && (!points || !point_id)) || n_visits < 0 || (n_visits > 0 && !visits) ||
      !(th > 0.f)) {
    set_error("%s: a null pointer, no key frame, a negative count or th <= 0", who);
    return VIEO_E_INVALID;
  }
  if (n_visits > kScwMaxVisits || (long long)n_points * n_visits > kScwMaxPointVisits) {
    set_error("%s: %d visits (limit %d) x %d points (limit on the product %lld)", who, n_visits, kScwMaxVisits, n_points,
              kScwMaxPointVisits);
    return VIEO_E_CAPACITY;
  }
  C.H.resize(n_kf);
  int rc;
  for (int f = 0; f < n_kf; ++f)
    if ((rc = loop_kf_prepare(kfs + f, kfs, who, f, C.H[f])) != VIEO_OK) return rc;
  for (int m = 0; m < n_points; ++m)
    if (point_id[m] < 0) {
      set_error("%s: point_id[%d] = %d is negative", who, m, point_id[m]);
      return VIEO_E_INVALID;
    }
  for (int v = 0; v < n_visits; ++v) {
    const Visit& V = visits[v];
    bool finite = true;
    for (int i = 0; i < 12; ++i) finite = finite && std::isfinite(V.Scw[i]);
    if (V.kf < 0 || V.kf >= n_kf || !finite || (V.Scw[0] == 0.f && V.Scw[1] == 0.f && V.Scw[2] == 0.f)) {
      set_error("%s: visit %d names key frame %d (of %d) or has a non-finite Scw or a zero first row", who, v, V.kf, n_kf);
      return VIEO_E_INVALID;
    }
  }
  C.nc = kfs->n_cams, C.n_points = n_points, C.n_visits = n_visits;
  return VIEO_OK;
}

// :510-515, Eigen float: scw by sqrtf of the row's dot product, float divisions, twcr = -(Rcrw^T tcrw)
void scw_decompose_eigen(const float* S, float* R, float* t, float* twcr) {
  const float scw = sqrtf((S[0] * S[0] + S[1] * S[1]) + S[2] * S[2]);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) R[r * 3 + c] = S[r * 4 + c] / scw;
    t[r] = S[r * 4 + 3] / scw;
  }
  for (int r = 0; r < 3; ++r) twcr[r] = -((R[r] * t[0] + R[3 + r] * t[1]) + R[6 + r] * t[2]);
}
// :1170-1173, cv::Mat (the arithmetic assumed in the header): dot and sqrt in double, scw rounded to float, every element
// times the double reciprocal rounded to float
void scw_decompose_cv(const float* S, float* R, float* t) {
  const double dot = ((double)S[0] * (double)S[0] + (double)S[1] * (double)S[1]) + (double)S[2] * (double)S[2];
  const float scw = (float)sqrt(dot);
  const double inv = 1.0 / (double)scw;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) R[r * 3 + c] = (float)((double)S[r * 4 + c] * inv);
    t[r] = (float)((double)S[r * 4 + 3] * inv);
  }
}

void scw_visit_dev(const LoopKfHost& dst, int slot, const float* R, const float* t, const float* centre, float th, ScwVisitDev& Q) {
  sim3_fuse_dev(dst, R, t, th, Q.fd);
  Q.fd.F.check_viewing_angle = 1;
  if (centre) memcpy(Q.fd.F.base.Ow, centre, sizeof(float) * 3);
  Q.dst = slot;
  for (int c = 0; c < kMaxCams; ++c) Q.cam_k0[c] = dst.k0[c];
}

// the device stage of a call: key frames side by side, grids, k_scw_gate, then k_scw_list (T.a = first, T.b = count,
// T.pool) or k_scw_best (T.a = best_idx, T.b = best_dist); keys come back as the key frames' own key indices
int scw_run(const ScwCall& C, const vieo_fuse_point* points, bool list, ScwTap& T) {
  int rc;
  const int nc = C.nc, n_items = C.n_visits * C.n_points * nc;
  KfStage& K = g_kf;
  Staging& S = K.s;
  K.open(C.H, false);
  const int zero[2] = {0, 0};
  const size_t o_vis = S.in(C.vis.data(), C.vis.size() * sizeof(ScwVisitDev));
  const size_t o_pts = S.in(points, (size_t)C.n_points * sizeof(vieo_fuse_point)), o_skip = S.in(C.skip.data(), C.skip.size() * 4);
  // [0] survivors, [1] listed candidates; the last input goes up as zeros and comes back in one copy with the results behind it
  const size_t o_ctr = S.in(zero, sizeof(zero));
  const size_t o_out = S.out((size_t)2 * n_items * 4);  // a, then b
  const size_t o_surv = S.scratch((size_t)n_items * sizeof(ScwSurvivor));
  int pool_cap = 0;
  if (list) {
    // (read at every call: the tests pin a small pool to reach the repeated launch)
    const char* e_pool = getenv("VIEO_SCW_POOL");
    const long pinned = e_pool ? strtol(e_pool, nullptr, 10) : 0;
    pool_cap = pinned > 0 ? (int)std::min<long long>(pinned, kScwMaxListed) : std::max(4096, 2 * n_items);
    if ((rc = K.pool.ensure((size_t)pool_cap * sizeof(ScwCand))) != VIEO_OK) return rc;
  }
  if ((rc = K.upload(0)) != VIEO_OK) return rc;
  const SbpGrid G = K.grid();
  const ScwVisitDev* d_vis = S.d<ScwVisitDev>(o_vis);
  const vieo_fuse_point* d_pts = S.d<vieo_fuse_point>(o_pts);
  ScwSurvivor* d_surv = S.d<ScwSurvivor>(o_surv);
  int32_t *d_a = S.d<int32_t>(o_out), *d_b = d_a + n_items;
  int* d_ctr = S.d<int>(o_ctr);
  const int* ctr = (const int*)S.h(o_ctr);  // as of the last download
  hipLaunchKernelGGL(k_scw_gate, dim3((n_items + 255) / 256), dim3(256), 0, 0, d_vis, n_items, C.n_points, nc, d_pts,
                     S.d<int>(o_skip), d_surv, d_ctr, d_a, list ? 0 : -1, d_b, list ? 0 : INT_MAX);
  const int n_blocks = std::min((n_items + 3) / 4, 2048);  // 256 CUs x 8 workgroups; the wavefronts stride over the survivors
  if (!list) {
    hipLaunchKernelGGL(k_scw_best, dim3(n_blocks), dim3(256), 0, 0, d_vis, C.n_points, nc, K.key_cap, G.cell_start, G.cell_rec,
                       K.desc(), d_pts, d_surv, d_ctr, d_a, d_b);
    VIEO_HIP_CHECK(hipGetLastError());
  }
  for (int attempt = 0; list; ++attempt) {
    hipLaunchKernelGGL(k_scw_list, dim3(n_blocks), dim3(256), 0, 0, d_vis, C.n_points, nc, K.key_cap, G.cell_start, G.cell_rec,
                       K.desc(), d_pts, d_surv, d_ctr, d_a, d_b, K.pool.as<ScwCand>(), pool_cap, d_ctr + 1);
    VIEO_HIP_CHECK(hipGetLastError());
    if ((rc = S.download(o_ctr, o_ctr + sizeof(zero), 0)) != VIEO_OK) return rc;
    if (ctr[1] < 0 || ctr[1] > kScwMaxListed) {
      set_error("SearchByProjection(Scw): more than %lld listed candidates in one call", kScwMaxListed);
      return VIEO_E_CAPACITY;
    }
    if (ctr[1] <= pool_cap) break;
    if (attempt == 1) {  // (the count of a window does not depend on the pool: not reached)
      set_error("SearchByProjection(Scw): the second listing counted %d entries, more than the first", ctr[1]);
      return VIEO_E_HIP;
    }
    // the pool was too small: ctr[1] is the exact total, the same survivors are listed again into a pool of that size
    pool_cap = ctr[1];
    if ((rc = K.pool.ensure((size_t)pool_cap * sizeof(ScwCand))) != VIEO_OK) return rc;
    VIEO_HIP_CHECK(hipMemsetAsync(d_ctr + 1, 0, 4, 0));
  }
  const size_t pool_bytes = (size_t)(list ? ctr[1] : 0) * sizeof(ScwCand);
  if ((rc = K.pool_pin.ensure(pool_bytes)) != VIEO_OK) return rc;
  if (pool_bytes) VIEO_HIP_CHECK(hipMemcpyAsync(K.pool_pin.p, K.pool.p, pool_bytes, hipMemcpyDeviceToHost, 0));
  if ((rc = S.download(o_ctr, 0)) != VIEO_OK) return rc;  // the counters and a, b; the wait covers the pool's copy
  const int32_t* h_out = (const int32_t*)S.h(o_out);
  T.a.assign(h_out, h_out + n_items), T.b.assign(h_out + n_items, h_out + 2 * (size_t)n_items);
  const ScwCand* h_pool = (const ScwCand*)K.pool_pin.p;
  T.pool.assign(h_pool, h_pool + (list ? ctr[1] : 0));
  for (int v = 0; v < C.n_visits; ++v) {  // position in the camera order -> key
    const int dst = C.vis[v].dst;
    const size_t i0 = (size_t)v * C.n_points * nc, i1 = i0 + (size_t)C.n_points * nc;
    for (size_t i = i0; i < i1; ++i) {
      const int c = (int)(i % nc);
      if (!list) {
        if (T.a[i] >= 0) T.a[i] = K.key(dst, c, T.a[i]);
      } else
        for (int e = 0; e < T.b[i]; ++e) T.pool[T.a[i] + e].key = K.key(dst, c, T.pool[T.a[i] + e].key);
    }
  }
  T.n_visits = C.n_visits, T.n_points = C.n_points, T.nc = nc;
  T.valid = true;
  g_scw_stats.valid = true, g_scw_stats.items = n_items, g_scw_stats.survivors = ctr[0];
  return VIEO_OK;
}

}  // namespace

extern "C" {

int vieo_search_by_projection_scw(const vieo_loop_keyframe* kfs, int n_kf, const vieo_fuse_point* points, const int32_t* point_id,
                                  int n_points, vieo_scw_visit* visits, int n_visits, float th) {
  static const char* who = "SearchByProjection(Scw)";
  ScwCall C;
  int rc = scw_check(who, kfs, n_kf, points, point_id, n_points, visits, n_visits, th, C);
  if (rc != VIEO_OK) return rc;
  for (int v = 0; v < n_visits; ++v)
    if (C.H[visits[v].kf].n > 0 && !visits[v].matched) {
      set_error("%s: visit %d has no matched array", who, v);
      return VIEO_E_INVALID;
    }
  if ((rc = require_device()) != VIEO_OK) return rc;
  ScwTap& T = g_scw_list_tap;
  T.valid = false;
  for (int v = 0; v < n_visits; ++v) visits[v].n_matches = 0;
  if (n_visits == 0 || n_points == 0) return VIEO_OK;
  const int nc = C.nc;
  C.vis.resize(n_visits);
  C.skip.assign((size_t)n_visits * n_points, 0);
  std::vector<int32_t> found;
  for (int v = 0; v < n_visits; ++v) {
    const vieo_scw_visit& V = visits[v];
    const LoopKfHost& h = C.H[V.kf];
    float R[9], t[3], twcr[3];
    scw_decompose_eigen(V.Scw, R, t, twcr);
    scw_visit_dev(h, V.kf, R, t, twcr, th, C.vis[v]);
    found.assign(V.matched, V.matched + h.n);  // spAlreadyFound (:518-519)
    std::sort(found.begin(), found.end());
    int* sk = C.skip.data() + (size_t)v * n_points;
    for (int m = 0; m < n_points; ++m)
      if ((points[m].skip_mask & (1u << 31)) || std::binary_search(found.begin(), found.end(), point_id[m])) sk[m] = INT_MIN;
  }
  if ((rc = scw_run(C, points, true, T)) != VIEO_OK) return rc;
  // :524-623 in the reference's order over the listed candidates
  for (int v = 0; v < n_visits; ++v) {
    vieo_scw_visit& V = visits[v];
    int n = 0;
    for (int m = 0; m < n_points; ++m)
      for (int c = 0; c < nc; ++c) {
        const size_t item = ((size_t)v * n_points + m) * nc + c;
        const ScwCand* cand = T.pool.data() + T.a[item];
        int best_dist = INT_MAX, best_idx = -1;
        for (int e = 0; e < T.b[item]; ++e)
          if (V.matched[cand[e].key] < 0 && cand[e].dist < best_dist) best_dist = cand[e].dist, best_idx = cand[e].key;
        if (best_idx >= 0) V.matched[best_idx] = point_id[m], n++;
      }
    V.n_matches = n;
  }
  return VIEO_OK;
}

int vieo_search_by_projection_scw_tap(int visit, int32_t* count, int32_t* key, int32_t* dist, int32_t* order, int cap) {
  const ScwTap& T = g_scw_list_tap;
  if (!T.valid) return VIEO_E_EMPTY;
  if (visit < 0 || visit >= T.n_visits || cap < 0) return VIEO_E_INVALID;
  const size_t n = (size_t)T.n_points * T.nc, i0 = (size_t)visit * n;
  for (size_t i = 0; i < n; ++i) {
    const int cnt = T.b[i0 + i];
    if (count) count[i] = cnt;
    const ScwCand* cand = T.pool.data() + T.a[i0 + i];
    for (int e = 0; e < std::min(cnt, cap); ++e) {
      if (key) key[i * cap + e] = cand[e].key;
      if (dist) dist[i * cap + e] = cand[e].dist;
      if (order) order[i * cap + e] = cand[e].order;
    }
  }
  return VIEO_OK;
}

int vieo_fuse_scw(const vieo_loop_keyframe* kfs, int n_kf, const vieo_fuse_point* points, const int32_t* point_id, int n_points,
                  vieo_fuse_scw_visit* visits, int n_visits, float th) {
  static const char* who = "Fuse(Scw)";
  ScwCall C;
  int rc = scw_check(who, kfs, n_kf, points, point_id, n_points, visits, n_visits, th, C);
  if (rc != VIEO_OK) return rc;
  for (int v = 0; v < n_visits; ++v)
    if (n_points > 0 && (!visits[v].match_key || !visits[v].replace || !visits[v].added)) {
      set_error("%s: visit %d has a null output array", who, v);
      return VIEO_E_INVALID;
    }
  if ((rc = require_device()) != VIEO_OK) return rc;
  ScwTap& T = g_scw_best_tap;
  T.valid = false;
  for (int v = 0; v < n_visits; ++v) visits[v].n_fused = 0;
  if (n_visits == 0 || n_points == 0) return VIEO_OK;
  const int nc = C.nc;
  C.vis.resize(n_visits);
  C.skip.assign((size_t)n_visits * n_points, 0);
  for (int v = 0; v < n_visits; ++v) {
    const vieo_fuse_scw_visit& V = visits[v];
    const LoopKfHost& h = C.H[V.kf];
    float R[9], t[3];
    scw_decompose_cv(V.Scw, R, t);
    scw_visit_dev(h, V.kf, R, t, nullptr, th, C.vis[v]);
    // vbAlreadyMatched1 as written at :1177-1187: the camera of KEY index iMP (0 past the keys); the bit is set when a key
    // of that camera holds the loop point
    int* sk = C.skip.data() + (size_t)v * n_points;
    for (int m = 0; m < n_points; ++m) {
      if (points[m].skip_mask & (1u << 31)) {
        sk[m] = INT_MIN;
        continue;
      }
      const int cami = m < h.n ? h.cam(m) : 0;
      const auto range = h.keys_of(point_id[m]);
      for (auto it = range.first; it != range.second; ++it)
        if (h.cam(it->second) == cami) sk[m] |= 1 << cami;
    }
  }
  if ((rc = scw_run(C, points, false, T)) != VIEO_OK) return rc;
  // :193-203 (MatchMultiCam, fuselater) and :1193-1217
  std::vector<int32_t> hold;
  for (int v = 0; v < n_visits; ++v) {
    vieo_fuse_scw_visit& V = visits[v];
    const LoopKfHost& h = C.H[V.kf];
    hold.assign(h.K->bow.mp_id, h.K->bow.mp_id + h.n);  // GetMapPoint(key) as this visit's AddMapPoint calls change it
    int n_fused = 0;
    for (int m = 0; m < n_points; ++m) {
      const size_t item = ((size_t)v * n_points + m) * nc;
      std::pair<int, int> set[kMaxCams];  // (key, camera), ascending by key
      int ns = 0;
      V.replace[m] = -1;
      for (int c = 0; c < nc; ++c) {
        const bool in = T.a[item + c] >= 0 && T.b[item + c] <= kThLow;
        V.match_key[(size_t)m * nc + c] = in ? T.a[item + c] : -1;
        V.added[(size_t)m * nc + c] = 0;
        if (in) set[ns++] = {T.a[item + c], c};
      }
      std::sort(set, set + ns);
      for (int e = 0; e < ns; ++e) {
        const int k = set[e].first;
        if (hold[k] >= 0)
          V.replace[m] = hold[k];
        else
          V.added[(size_t)m * nc + set[e].second] = 1, hold[k] = point_id[m];
        n_fused++;
      }
    }
    V.n_fused = n_fused;
  }
  return VIEO_OK;
}

int vieo_fuse_scw_tap(int visit, int32_t* best_idx, int32_t* best_dist) {
  const ScwTap& T = g_scw_best_tap;
  if (!T.valid) return VIEO_E_EMPTY;
  if (visit < 0 || visit >= T.n_visits) return VIEO_E_INVALID;
  const size_t n = (size_t)T.n_points * T.nc;
  if (best_idx && n) memcpy(best_idx, T.a.data() + (size_t)visit * n, n * 4);
  if (best_dist && n) memcpy(best_dist, T.b.data() + (size_t)visit * n, n * 4);
  return VIEO_OK;
}

int vieo_scw_gate_stats(int64_t* n_items, int64_t* n_survivors) {
  if (!g_scw_stats.valid) return VIEO_E_EMPTY;
  if (n_items) *n_items = g_scw_stats.items;
  if (n_survivors) *n_survivors = g_scw_stats.survivors;
  return VIEO_OK;
}

}  // extern "C"
