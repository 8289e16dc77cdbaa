// init_search.hip -- ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:628-723) for a batch of frame pairs.
//
// The reference is sequential over the keys of F1: a later key skips a key of F2 that an earlier one holds at a distance
// no larger (vMatchedDistance), or steals it.  Split as the Scw search of map_search.hip is:
//   sbp_build_grids  FrameBase::AssignFeaturesToGrid of every F2 (one camera, sbp_grid.h)                 [parallel]
//   k_init_list      one wavefront per octave-0 key of F1: GetFeaturesInArea(0, x, y, windowSize, 0, 0) of ITS pair's
//                    F2 in the reference's cell order, the Hamming distance (orb_match.h), and the LIST of the
//                    candidates that can change an outcome (below), in candidate order                     [parallel]
//   host             the walk through vMatchedDistance / vnMatches21 over the lists in key order, the rotation
//                    histogram with ComputeThreeMaxima, vbPrevMatched                                     [sequential]
//
// Which candidates come back.  A candidate enters the walk only through bestDist / bestDist2 (:667-673), and those are
// read twice: bestDist <= TH_LOW (:676) and bestDist < (float)bestDist2 * mfNNratio (:677).  A candidate with distance d
// can change the first only if d <= TH_LOW, and the second, given bestDist <= TH_LOW, only if NOT (TH_LOW < (float)d *
// mfNNratio): a larger d as bestDist2 passes the ratio test for every admissible bestDist, exactly as INT_MAX does.  The
// best and the second best of the candidates that are not skipped are order statistics, and the first key that attains the
// best is kept by dropping larger ones, so the walk over the list {d <= cut} gives the reference's decisions, with
//   cut = max(TH_LOW, the largest d with (float)d * mfNNratio <= (float)TH_LOW)            (init_cut below)
// For mfNNratio = 0.9: 55 * 0.9f = 49.5 <= 50 and 56 * 0.9f = 50.399998 > 50, so cut = 55.  The skip test
// vMatchedDistance[i2] <= dist (:665) needs no more: vMatchedDistance only ever holds a bestDist <= TH_LOW.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "common.h"
#include "sbp_grid.h"

namespace vieo {

struct InitQuery {
  float x, y;    // vbPrevMatched[i1]
  float r;       // (float)windowSize of the pair
  int pair;      // the F2 slot
};
struct InitCand {
  int key, dist, order;  // key of F2; order: position in the walk over ALL keys of the window's cells
};

// FrameBase::GetFeaturesInArea(0, x, y, r, 0, 0) (FrameBase.cpp:95-142) over the CSR grid of slot Q.pair, column by column
// with the lanes across a column's run.  hit(ok, dist, order, key) is called by EVERY lane once per 64 entries of a run (ok
// = false past the run's end, for an octave other than 0 or outside the window); every trip count is wave-uniform.
template <class Hit>
__device__ __forceinline__ void init_window_walk(const InitQuery& Q, const float* __restrict__ b, const int* __restrict__ cell_start,
                                                 const float4* __restrict__ cell_rec, const uint8_t* __restrict__ desc,
                                                 const uint4 d0, const uint4 d1, int lane, Hit&& hit) {
  const float x = Q.x, y = Q.y, r = Q.r;
  const float winv = (float)kGridCols / (b[1] - b[0]), hinv = (float)kGridRows / (b[3] - b[2]);
  const int min_cellx = max(0, (int)floorf((x - b[0] - r) * winv));
  const int max_cellx = min(kGridCols - 1, (int)ceilf((x - b[0] + r) * winv));
  const int min_celly = max(0, (int)floorf((y - b[2] - r) * hinv));
  const int max_celly = min(kGridRows - 1, (int)ceilf((y - b[2] + r) * hinv));
  if (min_cellx >= kGridCols || max_cellx < 0 || min_celly >= kGridRows || max_celly < 0) return;
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
        ok = oct == 0 && fabsf(k.x - x) < r && fabsf(k.y - y) < r;
        if (ok) d = (unsigned)hamming256(d0, d1, desc + (size_t)j * 32);
      }
      hit(ok, d, order + (e - s0), j);
    }
    order += s1 - s0;
  }
}

// One wavefront per query (the wavefronts of the grid stride over them): every window candidate with distance <= cut, in
// the reference's candidate order.  The window is walked twice, as k_scw_list does: the first walk counts, one atomic on
// *cursor reserves exactly that many entries of the pool, the second fills them.  A reservation past pool_cap writes
// nothing: the host reads *cursor = the exact total, makes the pool that large and launches again, so no list is cut.
__global__ void __launch_bounds__(256)
k_init_list(const InitQuery* __restrict__ qs, int n_q, const uint8_t* __restrict__ qdesc, SbpGridKeys gk, SbpGrid G,
            const uint8_t* __restrict__ desc, int cut, int32_t* __restrict__ list_first, int32_t* __restrict__ list_count,
            InitCand* __restrict__ pool, int pool_cap, int* __restrict__ cursor) {
  const int lane = threadIdx.x & 63, n_waves = gridDim.x * 4;
  const unsigned long long below = (1ull << lane) - 1ull;
  const float b[4] = {gk.bounds[0][0], gk.bounds[0][1], gk.bounds[0][2], gk.bounds[0][3]};
  for (int q = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); q < n_q; q += n_waves) {
    const InitQuery Q = qs[q];
    const int* cs = G.cell_start + (size_t)Q.pair * (kGridCells + 1);
    const float4* rec = G.cell_rec + (size_t)Q.pair * G.key_cap;
    const uint8_t* dsc = desc + (size_t)Q.pair * G.key_cap * 32;
    const uint4 d0 = ((const uint4*)(qdesc + (size_t)q * 32))[0], d1 = ((const uint4*)(qdesc + (size_t)q * 32))[1];
    int cnt = 0;
    init_window_walk(Q, b, cs, rec, dsc, d0, d1, lane,
                     [&](bool ok, unsigned d, int, int) { cnt += __popcll(__ballot(ok && d <= (unsigned)cut)); });
    if (lane == 0) list_first[q] = 0, list_count[q] = cnt;
    if (cnt == 0) continue;
    int first = 0;
    // the cursor saturates at INT_MAX instead of wrapping: every later reservation is refused and the host sees a total
    // beyond its limit
    if (lane == 0) {
      first = atomicAdd(cursor, cnt);
      if (first < 0 || first > INT_MAX - cnt) atomicExch(cursor, INT_MAX), first = INT_MAX;
      list_first[q] = first;
    }
    first = __shfl(first, 0);
    if (first > pool_cap - cnt) continue;  // (pool_cap >= cnt or the subtraction is negative: no wrap either way)
    int w = first;
    init_window_walk(Q, b, cs, rec, dsc, d0, d1, lane, [&](bool ok, unsigned d, int pos, int j) {
      const bool h = ok && d <= (unsigned)cut;
      const unsigned long long bal = __ballot(h);
      if (h) {
        InitCand c;
        c.key = j, c.dist = (int)d, c.order = pos;
        pool[w + __popcll(bal & below)] = c;
      }
      w += __popcll(bal);
    });
  }
}

}  // namespace vieo

using namespace vieo;

namespace {

const int kInitMaxPairs = 4096;
const long long kInitMaxListed = 1ll << 27;  // entries of the candidate pool (12 bytes each)

// the largest distance that can change an outcome (head of the file)
int init_cut(float nn_ratio) {
  int cut = kThLow;
  for (int d = kThLow + 1; d <= 256; ++d) {
    if (!((float)d * nn_ratio <= (float)kThLow)) break;
    cut = d;
  }
  return cut;
}

struct InitTap {
  bool valid = false;
  int n_pairs = 0;
  std::vector<int> n1;           // [pair]
  std::vector<size_t> q_first;   // [pair] first query of the pair
  std::vector<int32_t> q_of_key; // [pair's keys, concatenated]: the query of key i1, -1 for an octave above 0
  std::vector<size_t> key_first; // [pair] offset into q_of_key
  std::vector<int32_t> first, count;  // [query]
  std::vector<InitCand> pool;
};
thread_local InitTap g_init_tap;
thread_local Staging g_init_s;
thread_local DevBuf g_init_pool;
thread_local PinnedBuf g_init_pool_pin;

}  // namespace

extern "C" {

int vieo_search_for_initialization(vieo_init_pair* pairs, int n_pairs, const float* bounds, float nn_ratio, int check_orientation) {
  static const char* who = "SearchForInitialization";
  if (n_pairs < 0 || (n_pairs > 0 && !pairs) || !bounds || !(nn_ratio > 0.f) || !std::isfinite(nn_ratio)) {
    set_error("%s: a null pointer, a negative count or nn_ratio not a positive number", who);
    return VIEO_E_INVALID;
  }
  if (!(bounds[1] > bounds[0]) || !(bounds[3] > bounds[2]) || !std::isfinite(bounds[1] - bounds[0]) ||
      !std::isfinite(bounds[3] - bounds[2])) {
    set_error("%s: the image bounds are empty or not finite", who);
    return VIEO_E_INVALID;
  }
  if (n_pairs > kInitMaxPairs) {
    set_error("%s: %d pairs (limit %d)", who, n_pairs, kInitMaxPairs);
    return VIEO_E_CAPACITY;
  }
  int key_cap = 1;
  size_t n_q = 0, n_k1 = 0;
  for (int p = 0; p < n_pairs; ++p) {
    const vieo_init_pair& P = pairs[p];
    if (P.n1 < 0 || P.n2 < 0 || (P.n1 > 0 && (!P.keys1 || !P.desc1 || !P.prev_matched || !P.matches12)) ||
        (P.n2 > 0 && (!P.keys2 || !P.desc2)) || P.window_size < 0) {
      set_error("%s: pair %d has a null pointer, a negative key count or a negative window", who, p);
      return VIEO_E_INVALID;
    }
    if (P.n1 > kMaxKeys || P.n2 > kMaxKeys) {
      set_error("%s: pair %d has %d and %d keys (limit %d)", who, p, P.n1, P.n2, kMaxKeys);
      return VIEO_E_CAPACITY;
    }
    for (int i = 0; i < P.n1; ++i) {
      if (!std::isfinite(P.prev_matched[2 * i]) || !std::isfinite(P.prev_matched[2 * i + 1])) {
        set_error("%s: pair %d: prev_matched[%d] is not finite", who, p, i);
        return VIEO_E_INVALID;
      }
      n_q += P.keys1[i].octave <= 0;
    }
    for (int i = 0; i < P.n2; ++i) {
      const float a = P.keys2[i].angle;
      if (P.keys2[i].octave < 0 || P.keys2[i].octave > 0x7FFF || !std::isfinite(P.keys2[i].x) || !std::isfinite(P.keys2[i].y) ||
          !(a >= 0.f && a < 360.f)) {
        set_error("%s: pair %d: key %d of the second frame has an octave outside 0..32767, a non-finite position or an angle outside [0, 360)",
                  who, p, i);
        return VIEO_E_INVALID;
      }
    }
    for (int i = 0; i < P.n1; ++i)
      if (P.keys1[i].octave < 0 || !(P.keys1[i].angle >= 0.f && P.keys1[i].angle < 360.f)) {
        set_error("%s: pair %d: key %d of the first frame has a negative octave or an angle outside [0, 360)", who, p, i);
        return VIEO_E_INVALID;
      }
    key_cap = std::max(key_cap, P.n2);
    n_k1 += P.n1;
  }
  int rc;
  if ((rc = require_device()) != VIEO_OK) return rc;
  InitTap& T = g_init_tap;
  T.valid = false;
  const int cut = init_cut(nn_ratio);

  // ---- the queries (:642-648: the octave-0 keys of F1, in key order) and the second frames side by side
  Staging& S = g_init_s;
  S.reset();
  const size_t n_slots = (size_t)std::max(n_pairs, 1), n_k2 = n_slots * key_cap, nq_al = std::max<size_t>(n_q, 1);
  const int zero = 0;
  const size_t o_q = S.in(nullptr, nq_al * sizeof(InitQuery)), o_qd = S.in(nullptr, nq_al * 32);
  const size_t o_keys = S.in(nullptr, n_k2 * sizeof(vieo_keypoint)), o_desc = S.in(nullptr, n_k2 * 32);
  const size_t o_cf = S.in(nullptr, n_slots * 2 * 4);
  const size_t o_ctr = S.in(&zero, 4);  // the last input goes up as zero and comes back with the results behind it
  const size_t o_out = S.out(2 * nq_al * 4);  // first, then count
  const size_t o_ur = S.scratch(n_k2 * 4), o_cursor = S.scratch(n_slots * 4);
  const size_t o_start = S.scratch(n_slots * (kGridCells + 1) * 4), o_rec = S.scratch(n_k2 * sizeof(float4)), o_ang = S.scratch(n_k2 * 4);
  if ((rc = S.alloc()) != VIEO_OK) return rc;
  T.n_pairs = n_pairs;
  T.n1.resize(n_pairs), T.q_first.resize(n_pairs), T.key_first.resize(n_pairs), T.q_of_key.assign(n_k1, -1);
  {
    InitQuery* hq = S.hw<InitQuery>(o_q);
    uint8_t* hqd = S.hw<uint8_t>(o_qd);
    int* hcf = S.hw<int>(o_cf);
    size_t q = 0, k = 0;
    for (int p = 0; p < n_pairs; ++p) {
      const vieo_init_pair& P = pairs[p];
      T.n1[p] = P.n1, T.q_first[p] = q, T.key_first[p] = k;
      for (int i = 0; i < P.n1; ++i, ++k) {
        if (P.keys1[i].octave > 0) continue;
        hq[q] = InitQuery{P.prev_matched[2 * i], P.prev_matched[2 * i + 1], (float)P.window_size, p};
        memcpy(hqd + q * 32, P.desc1 + (size_t)i * 32, 32);
        T.q_of_key[k] = (int32_t)(q - T.q_first[p]);
        ++q;
      }
      if (P.n2) {
        memcpy(S.hw<vieo_keypoint>(o_keys) + (size_t)p * key_cap, P.keys2, (size_t)P.n2 * sizeof(vieo_keypoint));
        memcpy(S.hw<uint8_t>(o_desc) + (size_t)p * key_cap * 32, P.desc2, (size_t)P.n2 * 32);
      }
      hcf[2 * p] = 0, hcf[2 * p + 1] = P.n2;
    }
    if (n_pairs == 0) hcf[0] = hcf[1] = 0;
  }
  T.first.assign(n_q, 0), T.count.assign(n_q, 0), T.pool.clear();
  if (n_q > 0) {
    if ((rc = S.upload(0)) != VIEO_OK) return rc;
    VIEO_HIP_CHECK(hipMemsetAsync(S.d<float>(o_ur), 0xBF, n_k2 * 4, 0));  // a negative float in every key: monocular
    SbpGridKeys gk = {};
    gk.keys = S.d<vieo_keypoint>(o_keys), gk.uright = S.d<float>(o_ur), gk.cam_first = S.d<int>(o_cf), gk.cursor = S.d<int>(o_cursor);
    memcpy(gk.bounds[0], bounds, sizeof(float) * 4);
    const SbpGrid G = SbpGrid{S.d<int>(o_start), S.d<float4>(o_rec), S.d<float>(o_ang), key_cap, 1};
    if ((rc = sbp_build_grids(gk, n_pairs, G, 0)) != VIEO_OK) return rc;
    // (read at every call: the tests pin a small pool to reach the repeated launch)
    const char* e_pool = getenv("VIEO_INIT_POOL");
    const long pinned = e_pool ? strtol(e_pool, nullptr, 10) : 0;
    int pool_cap = pinned > 0 ? (int)std::min<long long>(pinned, kInitMaxListed)
                              : (int)std::min<long long>(kInitMaxListed, std::max<long long>(4096, 8 * (long long)n_q));
    if ((rc = g_init_pool.ensure((size_t)pool_cap * sizeof(InitCand))) != VIEO_OK) return rc;
    int* d_ctr = S.d<int>(o_ctr);
    const int* ctr = (const int*)S.h(o_ctr);  // as of the last download
    const int n_blocks = (int)std::min<size_t>((n_q + 3) / 4, 2048);  // 256 CUs x 8 workgroups; the wavefronts stride over the queries
    for (int attempt = 0;; ++attempt) {
      hipLaunchKernelGGL(k_init_list, dim3(n_blocks), dim3(256), 0, 0, S.d<InitQuery>(o_q), (int)n_q, S.d<uint8_t>(o_qd), gk, G,
                         S.d<uint8_t>(o_desc), cut, S.d<int32_t>(o_out), S.d<int32_t>(o_out) + nq_al, g_init_pool.as<InitCand>(), pool_cap,
                         d_ctr);
      VIEO_HIP_CHECK(hipGetLastError());
      if ((rc = S.download(o_ctr, o_ctr + 4, 0)) != VIEO_OK) return rc;
      if (ctr[0] < 0 || ctr[0] > kInitMaxListed) {
        set_error("%s: more than %lld listed candidates in one call", who, kInitMaxListed);
        return VIEO_E_CAPACITY;
      }
      if (ctr[0] <= pool_cap) break;
      if (attempt == 1) {  // (the count of a window does not depend on the pool: not reached)
        set_error("%s: the second listing counted %d entries, more than the first", who, ctr[0]);
        return VIEO_E_HIP;
      }
      pool_cap = ctr[0];
      if ((rc = g_init_pool.ensure((size_t)pool_cap * sizeof(InitCand))) != VIEO_OK) return rc;
      VIEO_HIP_CHECK(hipMemsetAsync(d_ctr, 0, 4, 0));
    }
    const size_t pool_bytes = (size_t)ctr[0] * sizeof(InitCand);
    if ((rc = g_init_pool_pin.ensure(pool_bytes)) != VIEO_OK) return rc;
    if (pool_bytes) VIEO_HIP_CHECK(hipMemcpyAsync(g_init_pool_pin.p, g_init_pool.p, pool_bytes, hipMemcpyDeviceToHost, 0));
    if ((rc = S.download(o_ctr, 0)) != VIEO_OK) return rc;  // the counter and first / count; the wait covers the pool's copy
    const int32_t* h_out = (const int32_t*)S.h(o_out);
    T.first.assign(h_out, h_out + n_q), T.count.assign(h_out + nq_al, h_out + nq_al + n_q);
    const InitCand* h_pool = (const InitCand*)g_init_pool_pin.p;
    T.pool.assign(h_pool, h_pool + ctr[0]);
  }
  T.valid = true;

  // ---- :630-722 in the reference's order over the listed candidates
  std::vector<int> matched_dist, matches21;
  std::vector<int> hist_key[kHistoLen];
  for (int p = 0; p < n_pairs; ++p) {
    vieo_init_pair& P = pairs[p];
    int nmatches = 0;
    std::fill_n(P.matches12, P.n1, -1);
    matched_dist.assign(P.n2, INT_MAX), matches21.assign(P.n2, -1);
    for (auto& h : hist_key) h.clear();
    const int32_t* qk = T.q_of_key.data() + T.key_first[p];
    for (int i1 = 0; i1 < P.n1; ++i1) {
      if (qk[i1] < 0) continue;
      const size_t q = T.q_first[p] + qk[i1];
      const InitCand* cand = T.pool.data() + T.first[q];
      int best = INT_MAX, best2 = INT_MAX, best_idx = -1;
      for (int e = 0; e < T.count[q]; ++e) {
        const int dist = cand[e].dist;
        if (matched_dist[cand[e].key] <= dist) continue;
        if (dist < best)
          best2 = best, best = dist, best_idx = cand[e].key;
        else if (dist < best2)
          best2 = dist;
      }
      if (best <= kThLow && (float)best < (float)best2 * nn_ratio) {
        if (matches21[best_idx] >= 0) P.matches12[matches21[best_idx]] = -1, nmatches--;
        P.matches12[i1] = best_idx, matches21[best_idx] = i1, matched_dist[best_idx] = best;
        nmatches++;
        if (check_orientation) hist_key[rot_bin(P.keys1[i1].angle, P.keys2[best_idx].angle)].push_back(i1);
      }
    }
    if (check_orientation) {
      int hist[kHistoLen];
      for (int b = 0; b < kHistoLen; ++b) hist[b] = (int)hist_key[b].size();  // (a stolen match stays counted, :693)
      const unsigned losers = three_maxima(hist);
      for (int b = 0; b < kHistoLen; ++b)
        if (losers >> b & 1)
          for (int i1 : hist_key[b])
            if (P.matches12[i1] >= 0) P.matches12[i1] = -1, nmatches--;
    }
    for (int i1 = 0; i1 < P.n1; ++i1)
      if (P.matches12[i1] >= 0) {
        P.prev_matched[2 * i1] = P.keys2[P.matches12[i1]].x;
        P.prev_matched[2 * i1 + 1] = P.keys2[P.matches12[i1]].y;
      }
    P.n_matches = nmatches;
  }
  return VIEO_OK;
}

int vieo_search_for_initialization_tap(int pair, int32_t* count, int32_t* key, int32_t* dist, int32_t* order, int cap) {
  const InitTap& T = g_init_tap;
  if (!T.valid) return VIEO_E_EMPTY;
  if (pair < 0 || pair >= T.n_pairs || cap < 0) return VIEO_E_INVALID;
  const int32_t* qk = T.q_of_key.data() + T.key_first[pair];
  for (int i = 0; i < T.n1[pair]; ++i) {
    if (qk[i] < 0) {
      if (count) count[i] = 0;
      continue;
    }
    const size_t q = T.q_first[pair] + qk[i];
    const int cnt = T.count[q];
    if (count) count[i] = cnt;
    const InitCand* cand = T.pool.data() + T.first[q];
    for (int e = 0; e < std::min(cnt, cap); ++e) {
      if (key) key[(size_t)i * cap + e] = cand[e].key;
      if (dist) dist[(size_t)i * cap + e] = cand[e].dist;
      if (order) order[(size_t)i * cap + e] = cand[e].order;
    }
  }
  return VIEO_OK;
}

}  // extern "C"
