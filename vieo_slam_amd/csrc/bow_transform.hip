// bow_transform.hip -- FrameBase::ComputeBoW (reference src/FrameBase.cpp:83-93 -> TemplatedVocabulary::transform(features,
// v, fv, levelsup), loop/DBoW2/DBoW2/TemplatedVocabulary.h:1007-1129; BowVector.cpp:34-84) for a batch of frames.
//   k_bow_descend  the greedy descent of every key of every frame.  VIEO_BOW_LANES (32 or 1) lanes per key: with 32 each
//                  lane takes one child (k <= 20), the level's winner is a min over (distance << 8 | child) -- DPP inside
//                  the rows of 16, one cross-lane permute between the two rows --, so the first child wins ties as the
//                  reference's strict < does.  With 1 a lane walks the children itself.
//   k_bow_pack     one workgroup per (frame, vector): bitonic sort of (id, key index) in LDS, run heads by a block scan,
//                  then mBowVec (word id, summed weight, L1-normalised) or mFeatVec (node id, node_first, node_feat).
// Bounds: a frame holds at most VIEO_BOW_MAX_KEYS keys (the LDS arrays of k_bow_pack); every device index is below the
// batch's key count, every tree index below n_nodes + 1 (validated when the vocabulary is built).
#include <vector>

#include "orb_match.h"
#include "vocabulary.h"
#include "wave_ops.h"

#ifndef VIEO_BOW_LANES
#define VIEO_BOW_LANES 32
#endif

namespace vieo {

static const uint32_t kBowNone = 0xFFFFFFFFu;  // a stopped word / padding: sorts behind every id
static const int kPackThreads = 512;

// nid_level = L - levelsup.  word[key] = kBowNone for a stopped word.
template <int G>
__global__ void __launch_bounds__(256)
k_bow_descend(const VocNode* __restrict__ nodes, const uint4* __restrict__ desc, const uint4* __restrict__ keys, int n_keys,
              int nid_level, uint32_t* __restrict__ word, uint32_t* __restrict__ node, double* __restrict__ weight) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int key = t / G, sub = t % G;
  if (key >= n_keys) return;  // (uniform over the G lanes of a key)
  const uint4 a0 = keys[2 * (size_t)key], a1 = keys[2 * (size_t)key + 1];
  VocNode N = nodes[0];
  uint32_t nid = 0;
  int level = 0;
  do {
    ++level;
    unsigned best = kBowNone;
    if (G == 1) {
      for (int c = 0; c < N.child_count; c++)
        best = min(best, ((unsigned)hamming256(a0, a1, desc + 2 * (size_t)(N.child_first + c)) << 8) | (unsigned)c);
    } else {
      if (sub < N.child_count)
        best = ((unsigned)hamming256(a0, a1, desc + 2 * (size_t)(N.child_first + sub)) << 8) | (unsigned)sub;
      best = min(best, (unsigned)VIEO_DPP(best, best, VIEO_DPP_QUAD_XOR1, 0xF));
      best = min(best, (unsigned)VIEO_DPP(best, best, VIEO_DPP_QUAD_XOR2, 0xF));
      best = min(best, (unsigned)VIEO_DPP(best, best, VIEO_DPP_ROW_HALF_MIRROR, 0xF));
      best = min(best, (unsigned)VIEO_DPP(best, best, VIEO_DPP_ROW_MIRROR, 0xF));
      best = min(best, (unsigned)__shfl_xor((int)best, 16));
    }
    N = nodes[N.child_first + (int)(best & 255u)];
    if (level == nid_level) nid = N.node_id;
  } while (N.child_count > 0);
  if (level < nid_level) nid = N.node_id;  // a leaf above level L - levelsup reports itself
  if (sub == 0) {
    word[key] = N.weight > 0 ? (uint32_t)N.word_id : kBowNone;
    node[key] = nid;
    weight[key] = N.weight;
  }
}

struct BowPackOut {
  int32_t* counts;      // [n_frames][2] n_words, n_nodes
  uint32_t* word_id;    // [n_keys_all]
  double* word_value;   // [n_keys_all]
  uint32_t* node_id;    // [n_keys_all]
  int32_t* node_first;  // [n_keys_all + n_frames]: frame f at key_off[f] + f
  int32_t* node_feat;   // [n_keys_all]
};

// blockIdx.x = frame, blockIdx.y = 0: mBowVec, 1: mFeatVec
__global__ void __launch_bounds__(kPackThreads)
k_bow_pack(const int* __restrict__ key_off, const uint32_t* __restrict__ word, const uint32_t* __restrict__ node,
           const double* __restrict__ weight, BowPackOut out) {
  __shared__ uint32_t s_id[VIEO_BOW_MAX_KEYS];
  __shared__ uint16_t s_ix[VIEO_BOW_MAX_KEYS];
  __shared__ int s_scan[kPackThreads];
  __shared__ double s_red[kPackThreads / 64];
  __shared__ int s_valid;
  const int f = blockIdx.x, t = threadIdx.x;
  const bool words = blockIdx.y == 0;
  const int base = key_off[f], n = key_off[f + 1] - base;
  int npad = 1;
  while (npad < n) npad <<= 1;
  const uint32_t* src = (words ? word : node) + base;
  for (int i = t; i < npad; i += kPackThreads) {
    // a stopped word leaves both vectors
    s_id[i] = i < n && word[base + i] != kBowNone ? src[i] : kBowNone;
    s_ix[i] = (uint16_t)i;
  }
  if (t == 0) s_valid = 0;
  __syncthreads();
  for (int k = 2; k <= npad; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int p = t; p < (npad >> 1); p += kPackThreads) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), x = i | j;  // the pair (i, i ^ j), i < x
        const uint32_t ai = s_id[i], ax = s_id[x];
        const uint16_t bi = s_ix[i], bx = s_ix[x];
        const bool gt = ai > ax || (ai == ax && bi > bx);
        if (gt == ((i & k) == 0)) s_id[i] = ax, s_id[x] = ai, s_ix[i] = bx, s_ix[x] = bi;
      }
      __syncthreads();
    }
  for (int i = t; i < npad; i += kPackThreads)
    if (s_id[i] != kBowNone && (i + 1 == npad || s_id[i + 1] == kBowNone)) s_valid = i + 1;
  __syncthreads();
  const int nv = s_valid;
  // run heads: thread t owns [lo, hi)
  const int chunk = (nv + kPackThreads - 1) / kPackThreads;
  const int lo = min(t * chunk, nv), hi = min(lo + chunk, nv);
  int heads = 0;
  for (int i = lo; i < hi; i++) heads += i == 0 || s_id[i] != s_id[i - 1];
  s_scan[t] = heads;
  __syncthreads();
  for (int off = 1; off < kPackThreads; off <<= 1) {
    const int v = t >= off ? s_scan[t - off] : 0;
    __syncthreads();
    s_scan[t] += v;
    __syncthreads();
  }
  const int total = s_scan[kPackThreads - 1];
  int r = s_scan[t] - heads;
  if (words) {
    double part = 0;
    for (int i = lo; i < hi; i++) {
      if (!(i == 0 || s_id[i] != s_id[i - 1])) continue;
      const double w = weight[base + s_ix[i]];
      double v = w;  // v.addWeight once per occurrence
      for (int j = i + 1; j < nv && s_id[j] == s_id[i]; j++) v += w;
      out.word_id[base + r] = s_id[i];
      out.word_value[base + r] = v;
      part += v;
      r++;
    }
    part = wave_sum_f64(part);
    if ((t & 63) == 0) s_red[t >> 6] = part;
    __syncthreads();
    double norm = 0;
    for (int w = 0; w < kPackThreads / 64; w++) norm += s_red[w];
    if (norm > 0)
      for (int i = t; i < total; i += kPackThreads) out.word_value[base + i] /= norm;
    if (t == 0) out.counts[2 * f] = total;
  } else {
    int32_t* nfirst = out.node_first + base + f;
    for (int i = lo; i < hi; i++) {
      out.node_feat[base + i] = s_ix[i];
      if (i == 0 || s_id[i] != s_id[i - 1]) {
        out.node_id[base + r] = s_id[i];
        nfirst[r] = i;
        r++;
      }
    }
    if (t == 0) nfirst[total] = nv, out.counts[2 * f + 1] = total;
  }
}

struct BowTransformScratch {
  PinnedBuf pin;
  DevBuf dev;
};
static thread_local BowTransformScratch g_bowt;

}  // namespace vieo

extern "C" int vieo_bow_transform(const vieo_vocabulary* voc, const vieo_bow_frame* frames, int n_frames, int levelsup,
                                  vieo_bow_vectors* out) {
  using namespace vieo;
  if (!voc || !frames || !out || n_frames <= 0) return VIEO_E_INVALID;
  size_t N = 0;
  for (int f = 0; f < n_frames; f++) {
    const vieo_bow_frame& F = frames[f];
    const vieo_bow_vectors& O = out[f];
    if (F.n_keys < 0 || (F.n_keys > 0 && (!F.descriptors || !O.word_id || !O.word_value || !O.node_id || !O.node_feat)) ||
        !O.node_first) {
      set_error("bow_transform: frame %d: a null pointer or n_keys < 0", f);
      return VIEO_E_INVALID;
    }
    N += (size_t)F.n_keys;
  }
  for (int f = 0; f < n_frames; f++)
    if (frames[f].n_keys > VIEO_BOW_MAX_KEYS) {
      set_error("bow_transform: frame %d has %d keys, at most %d", f, frames[f].n_keys, VIEO_BOW_MAX_KEYS);
      return VIEO_E_CAPACITY;
    }
  if (N > ((size_t)1 << 30)) return VIEO_E_CAPACITY;
  int rc = require_device();
  if (rc != VIEO_OK) return rc;
  if (N == 0 || voc->n_words == 0) {  // transform() of an empty vocabulary clears both vectors
    for (int f = 0; f < n_frames; f++) out[f].n_words = out[f].n_nodes = 0, out[f].node_first[0] = 0;
    return VIEO_OK;
  }
  // one block: [key_off | descriptors] up, [word | node | weight] scratch, [counts | node_first | node_feat | word_id |
  // node_id | word_value] back
  auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t o_off = 0, o_desc = al((n_frames + 1) * 4), o_word = o_desc + al(N * 32), o_node = o_word + al(N * 4),
               o_wt = o_node + al(N * 4), o_cnt = o_wt + al(N * 8), o_nfirst = o_cnt + al((size_t)n_frames * 8),
               o_nfeat = o_nfirst + al((N + n_frames) * 4), o_wid = o_nfeat + al(N * 4), o_nid = o_wid + al(N * 4),
               o_wval = o_nid + al(N * 4), total = o_wval + al(N * 8);
  BowTransformScratch& S = g_bowt;
  if ((rc = S.pin.ensure(total)) != VIEO_OK || (rc = S.dev.ensure(total)) != VIEO_OK) return rc;
  uint8_t* hp = (uint8_t*)S.pin.p;
  uint8_t* dp = (uint8_t*)S.dev.p;
  int* key_off = (int*)(hp + o_off);
  key_off[0] = 0;
  for (int f = 0; f < n_frames; f++) {
    if (frames[f].n_keys) memcpy(hp + o_desc + 32 * (size_t)key_off[f], frames[f].descriptors, 32 * (size_t)frames[f].n_keys);
    key_off[f + 1] = key_off[f] + frames[f].n_keys;
  }
  hipStream_t st = nullptr;
  VIEO_HIP_CHECK(hipMemcpyAsync(dp, hp, o_desc + N * 32, hipMemcpyHostToDevice, st));
  const size_t lanes = N * VIEO_BOW_LANES;
  hipLaunchKernelGGL(k_bow_descend<VIEO_BOW_LANES>, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, voc->d_nodes,
                     (const uint4*)voc->d_desc, (const uint4*)(dp + o_desc), (int)N, voc->L - levelsup,
                     (uint32_t*)(dp + o_word), (uint32_t*)(dp + o_node), (double*)(dp + o_wt));
  VIEO_HIP_CHECK(hipGetLastError());
  BowPackOut P{(int32_t*)(dp + o_cnt), (uint32_t*)(dp + o_wid), (double*)(dp + o_wval),
               (uint32_t*)(dp + o_nid), (int32_t*)(dp + o_nfirst), (int32_t*)(dp + o_nfeat)};
  hipLaunchKernelGGL(k_bow_pack, dim3(n_frames, 2), dim3(kPackThreads), 0, st, (const int*)(dp + o_off),
                     (const uint32_t*)(dp + o_word), (const uint32_t*)(dp + o_node), (const double*)(dp + o_wt), P);
  VIEO_HIP_CHECK(hipGetLastError());
  VIEO_HIP_CHECK(hipMemcpyAsync(hp + o_cnt, dp + o_cnt, total - o_cnt, hipMemcpyDeviceToHost, st));
  VIEO_HIP_CHECK(hipStreamSynchronize(st));
  const int32_t* cnt = (const int32_t*)(hp + o_cnt);
  for (int f = 0; f < n_frames; f++) {
    vieo_bow_vectors& O = out[f];
    const size_t b = key_off[f];
    const int nw = cnt[2 * f], nn = cnt[2 * f + 1];
    O.n_words = nw, O.n_nodes = nn;
    if (frames[f].n_keys == 0) {
      O.node_first[0] = 0;
      continue;
    }
    memcpy(O.word_id, hp + o_wid + 4 * b, 4 * (size_t)nw);
    memcpy(O.word_value, hp + o_wval + 8 * b, 8 * (size_t)nw);
    memcpy(O.node_id, hp + o_nid + 4 * b, 4 * (size_t)nn);
    memcpy(O.node_first, hp + o_nfirst + 4 * (b + f), 4 * (size_t)(nn + 1));
    memcpy(O.node_feat, hp + o_nfeat + 4 * b, 4 * (size_t)((const int32_t*)(hp + o_nfirst))[b + f + nn]);
  }
  return VIEO_OK;
}
