// kf_database.hip -- KeyFrameDatabase (reference src/KeyFrameDatabase.cc) with the scoring on the device.
//   k_kfdb_score  one wavefront per stored key frame: its lanes stride over the key frame's words, each looks its word up
//                 in the query (ids resident in LDS, binary search) and accumulates the number of shared words, the
//                 smallest shared word id and the terms of L1Scoring::score (ScoringObject.cpp:23-68) in double.
//   host          what the inverted file's walk amounts to -- the key frames that share a word, in ascending (smallest
//                 shared word id, insertion sequence) -- and the sequential tail of Detect*Candidates.
// The key frames' vectors live in one device CSR (appended on add, compacted when half of it is dead); the host keeps a
// mirror to re-upload from when the buffer grows.
// Bounds: a query holds at most VIEO_BOW_MAX_KEYS words (s_q); a row's [first, first + count) lies inside the CSR by
// construction (rows are made from the mirror's offsets only).
#include <algorithm>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "vocabulary.h"
#include "wave_ops.h"

namespace vieo {

struct KfdbRow {
  int64_t first;  // offset into the CSR
  int32_t count, pad;
};  // 16 bytes
struct KfdbScore {
  int32_t n_common;
  uint32_t first_word;  // 0xFFFFFFFF: shares nothing
  double score;
};  // 16 bytes

__global__ void __launch_bounds__(256)
k_kfdb_score(const KfdbRow* __restrict__ rows, int n_rows, const uint32_t* __restrict__ words,
             const double* __restrict__ values, const uint32_t* __restrict__ q_id, const double* __restrict__ q_val, int nq,
             KfdbScore* __restrict__ out) {
  __shared__ uint32_t s_q[VIEO_BOW_MAX_KEYS];
  for (int i = threadIdx.x; i < nq; i += 256) s_q[i] = q_id[i];
  __syncthreads();
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n_rows) return;  // (uniform over the wavefront)
  const KfdbRow R = rows[row];
  int common = 0;
  unsigned first = 0xFFFFFFFFu;
  double sum = 0;
  for (int i = lane; i < R.count; i += 64) {
    const uint32_t w = words[R.first + i];
    int lo = 0, hi = nq;  // lower bound of w in the query
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_q[mid] < w)
        lo = mid + 1;
      else
        hi = mid;
    }
    if (lo < nq && s_q[lo] == w) {
      const double vi = q_val[lo], wi = values[R.first + i];
      sum += fabs(vi - wi) - fabs(vi) - fabs(wi);
      common++;
      first = min(first, w);
    }
  }
  common = wave_sum_i32(common);
  first = wave_min_u32(first);
  sum = wave_sum_f64(sum);
  if (lane == 0) out[row] = KfdbScore{common, first, -sum / 2.0};
}

struct KfdbEntry {
  int64_t id;
  int64_t seq;
  size_t first;
  int count;
  float reloc_score = 0.f, loop_score = 0.f;  // mRelocScore / mLoopScore (defined as 0 before the first write)
  int n_covis = 0;
  int64_t covis[10];
};

}  // namespace vieo

struct vieo_kfdb {
  int n_voc_words = 0;
  std::vector<vieo::KfdbEntry> kfs;  // stored key frames in insertion order
  std::unordered_map<int64_t, int> index;  // id -> position in kfs
  int64_t next_seq = 0;
  std::vector<uint32_t> words;  // the CSR's mirror
  std::vector<double> values;
  size_t dead = 0, uploaded = 0;
  vieo::DevBuf d_words, d_values, d_rows, d_out, d_q;
  std::vector<vieo::KfdbScore> last;  // the last query's table, per kfs position
  bool last_valid = false;
};

namespace vieo {

static void kfdb_reindex(vieo_kfdb* D) {
  D->index.clear();
  for (size_t i = 0; i < D->kfs.size(); i++) D->index[D->kfs[i].id] = (int)i;
}

static void kfdb_compact(vieo_kfdb* D) {
  std::vector<uint32_t> w;
  std::vector<double> v;
  w.reserve(D->words.size() - D->dead), v.reserve(D->words.size() - D->dead);
  for (KfdbEntry& e : D->kfs) {
    const size_t first = w.size();
    w.insert(w.end(), D->words.begin() + e.first, D->words.begin() + e.first + e.count);
    v.insert(v.end(), D->values.begin() + e.first, D->values.begin() + e.first + e.count);
    e.first = first;
  }
  D->words.swap(w), D->values.swap(v);
  D->dead = 0, D->uploaded = 0;
}

static int kfdb_query_ok(const vieo_kfdb* D, const uint32_t* word_id, const double* word_value, int n) {
  if (!D || n < 0 || (n > 0 && (!word_id || !word_value))) return VIEO_E_INVALID;
  if (n > VIEO_BOW_MAX_KEYS) {
    set_error("kfdb: a query of %d words, at most %d", n, VIEO_BOW_MAX_KEYS);
    return VIEO_E_CAPACITY;
  }
  for (int i = 1; i < n; i++)
    if (word_id[i] <= word_id[i - 1]) {
      set_error("kfdb: the query's words do not ascend at %d", i);
      return VIEO_E_INVALID;
    }
  return VIEO_OK;
}

// scores of the key frames at positions pos[0..n) of D->kfs against the query
static int kfdb_run(vieo_kfdb* D, const uint32_t* word_id, const double* word_value, int nq, const int* pos, int n,
                    std::vector<KfdbScore>& out) {
  out.assign(n, KfdbScore{0, 0xFFFFFFFFu, 0.0});
  if (n == 0 || nq == 0) return VIEO_OK;  // score() of an empty vector is 0
  int rc = require_device();
  if (rc != VIEO_OK) return rc;
  const size_t total = D->words.size();
  const void* w_before = D->d_words.p;
  const void* v_before = D->d_values.p;
  const size_t w_cap = D->d_words.cap, v_cap = D->d_values.cap;
  if ((rc = D->d_words.ensure(std::max<size_t>(total, 1) * 4)) != VIEO_OK ||
      (rc = D->d_values.ensure(std::max<size_t>(total, 1) * 8)) != VIEO_OK) {
    D->uploaded = 0;
    return rc;
  }
  if (D->d_words.p != w_before || D->d_words.cap != w_cap || D->d_values.p != v_before || D->d_values.cap != v_cap)
    D->uploaded = 0;  // a grown buffer is a new one
  if (D->uploaded < total) {
    VIEO_HIP_CHECK(hipMemcpy(D->d_words.as<uint32_t>() + D->uploaded, D->words.data() + D->uploaded,
                             (total - D->uploaded) * 4, hipMemcpyHostToDevice));
    VIEO_HIP_CHECK(hipMemcpy(D->d_values.as<double>() + D->uploaded, D->values.data() + D->uploaded,
                             (total - D->uploaded) * 8, hipMemcpyHostToDevice));
    D->uploaded = total;
  }
  std::vector<KfdbRow> rows(n);
  for (int i = 0; i < n; i++) rows[i] = KfdbRow{(int64_t)D->kfs[pos[i]].first, D->kfs[pos[i]].count, 0};
  if ((rc = D->d_rows.ensure((size_t)n * sizeof(KfdbRow))) != VIEO_OK ||
      (rc = D->d_out.ensure((size_t)n * sizeof(KfdbScore))) != VIEO_OK || (rc = D->d_q.ensure((size_t)nq * 12 + 8)) != VIEO_OK)
    return rc;
  double* dq_val = D->d_q.as<double>();
  uint32_t* dq_id = (uint32_t*)(dq_val + nq);
  VIEO_HIP_CHECK(hipMemcpy(D->d_rows.p, rows.data(), (size_t)n * sizeof(KfdbRow), hipMemcpyHostToDevice));
  VIEO_HIP_CHECK(hipMemcpy(dq_val, word_value, (size_t)nq * 8, hipMemcpyHostToDevice));
  VIEO_HIP_CHECK(hipMemcpy(dq_id, word_id, (size_t)nq * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_kfdb_score, dim3((n + 3) / 4), dim3(256), 0, nullptr, D->d_rows.as<KfdbRow>(), n,
                     D->d_words.as<uint32_t>(), D->d_values.as<double>(), dq_id, dq_val, nq, D->d_out.as<KfdbScore>());
  VIEO_HIP_CHECK(hipGetLastError());
  VIEO_HIP_CHECK(hipMemcpy(out.data(), D->d_out.p, (size_t)n * sizeof(KfdbScore), hipMemcpyDeviceToHost));
  return VIEO_OK;
}

// Detect{Relocalization,Loop}Candidates after the inverted file's walk.  loop: connected key frames are not listed and
// never count as neighbours, a neighbour must itself have been scored in this query, bestAccScore starts at min_score.
static int kfdb_detect(vieo_kfdb* D, const uint32_t* word_id, const double* word_value, int nq, bool loop,
                       const int64_t* connected, int n_connected, float min_score, int64_t* out_ids, int capacity,
                       int32_t* n_out) {
  int rc = kfdb_query_ok(D, word_id, word_value, nq);
  if (rc != VIEO_OK) return rc;
  if (!n_out || capacity < 0 || (capacity > 0 && !out_ids) || (loop && n_connected > 0 && !connected) || n_connected < 0)
    return VIEO_E_INVALID;
  const int n = (int)D->kfs.size();
  std::vector<int> pos(n);
  for (int i = 0; i < n; i++) pos[i] = i;
  std::vector<KfdbScore> sc;
  if ((rc = kfdb_run(D, word_id, word_value, nq, pos.data(), n, sc)) != VIEO_OK) return rc;
  std::unordered_set<int64_t> conn;
  if (loop) conn.insert(connected, connected + n_connected);
  // lKFsSharingWords: first met while walking the query's words ascending, each word's list in insertion order
  std::vector<int> listed;
  std::vector<uint8_t> is_listed(n, 0);
  for (int i = 0; i < n; i++)
    if (sc[i].n_common > 0 && !(loop && conn.count(D->kfs[i].id))) listed.push_back(i), is_listed[i] = 1;
  std::sort(listed.begin(), listed.end(), [&](int a, int b) {
    return sc[a].first_word != sc[b].first_word ? sc[a].first_word < sc[b].first_word : D->kfs[a].seq < D->kfs[b].seq;
  });
  std::vector<float> score(n);  // the member after this query: written only where the reference writes it
  for (int i = 0; i < n; i++) score[i] = loop ? D->kfs[i].loop_score : D->kfs[i].reloc_score;
  std::vector<int64_t> result;
  if (!listed.empty()) {
    int maxCommonWords = 0;
    for (int i : listed) maxCommonWords = std::max(maxCommonWords, sc[i].n_common);
    const int minCommonWords = (int)((float)maxCommonWords * 0.8f);
    std::vector<std::pair<float, int>> lScoreAndMatch;
    for (int i : listed)
      if (sc[i].n_common > minCommonWords) {
        const float si = (float)sc[i].score;
        score[i] = si;
        if (!loop || si >= min_score) lScoreAndMatch.push_back({si, i});
      }
    std::vector<std::pair<float, int>> lAccScoreAndMatch;
    float bestAccScore = loop ? min_score : 0.f;
    for (const auto& sm : lScoreAndMatch) {
      const KfdbEntry& E = D->kfs[sm.second];
      float bestScore = sm.first, accScore = sm.first;
      int best = sm.second;
      for (int c = 0; c < E.n_covis; c++) {
        auto it = D->index.find(E.covis[c]);
        if (it == D->index.end()) continue;  // erased or never added: no query stamp
        const int j = it->second;
        if (loop ? !(is_listed[j] && sc[j].n_common > minCommonWords) : sc[j].n_common == 0) continue;
        accScore += score[j];
        if (score[j] > bestScore) best = j, bestScore = score[j];
      }
      lAccScoreAndMatch.push_back({accScore, best});
      if (accScore > bestAccScore) bestAccScore = accScore;
    }
    const float minScoreToRetain = 0.75f * bestAccScore;
    std::vector<uint8_t> added(n, 0);
    for (const auto& am : lAccScoreAndMatch)
      if (am.first > minScoreToRetain && !added[am.second]) result.push_back(D->kfs[am.second].id), added[am.second] = 1;
  }
  *n_out = (int32_t)result.size();
  if ((int)result.size() > capacity) {
    set_error("kfdb: %d candidates, room for %d", (int)result.size(), capacity);
    return VIEO_E_CAPACITY;
  }
  for (int i = 0; i < n; i++) (loop ? D->kfs[i].loop_score : D->kfs[i].reloc_score) = score[i];
  std::copy(result.begin(), result.end(), out_ids);
  D->last.swap(sc), D->last_valid = true;
  return VIEO_OK;
}

}  // namespace vieo

extern "C" int vieo_kfdb_create(vieo_kfdb** out, const vieo_vocabulary* voc) {
  if (!out || !voc) return VIEO_E_INVALID;
  vieo_kfdb* D = new vieo_kfdb;
  D->n_voc_words = voc->n_words;
  *out = D;
  return VIEO_OK;
}

extern "C" void vieo_kfdb_destroy(vieo_kfdb* db) {
  if (!db) return;
  db->d_words.release(), db->d_values.release(), db->d_rows.release(), db->d_out.release(), db->d_q.release();
  delete db;
}

extern "C" int vieo_kfdb_clear(vieo_kfdb* db) {
  if (!db) return VIEO_E_INVALID;
  db->kfs.clear(), db->index.clear(), db->words.clear(), db->values.clear();
  db->dead = db->uploaded = 0, db->last_valid = false;
  return VIEO_OK;
}

extern "C" int vieo_kfdb_size(const vieo_kfdb* db) { return db ? (int)db->kfs.size() : VIEO_E_INVALID; }

extern "C" int vieo_kfdb_add(vieo_kfdb* db, int64_t kf_id, const uint32_t* word_id, const double* word_value, int n_words) {
  using namespace vieo;
  if (!db || n_words < 0 || (n_words > 0 && (!word_id || !word_value))) return VIEO_E_INVALID;
  if (db->index.count(kf_id)) {
    set_error("kfdb: key frame %lld is already stored", (long long)kf_id);
    return VIEO_E_INVALID;
  }
  for (int i = 0; i < n_words; i++)
    if ((i > 0 && word_id[i] <= word_id[i - 1]) || word_id[i] >= (uint32_t)db->n_voc_words) {
      set_error("kfdb: key frame %lld: word %d (%u) does not ascend or is not of the vocabulary", (long long)kf_id, i, word_id[i]);
      return VIEO_E_INVALID;
    }
  KfdbEntry e;
  e.id = kf_id, e.seq = db->next_seq++, e.first = db->words.size(), e.count = n_words;
  db->words.insert(db->words.end(), word_id, word_id + n_words);
  db->values.insert(db->values.end(), word_value, word_value + n_words);
  db->index[kf_id] = (int)db->kfs.size();
  db->kfs.push_back(e);
  db->last_valid = false;
  return VIEO_OK;
}

extern "C" int vieo_kfdb_erase(vieo_kfdb* db, int64_t kf_id) {
  using namespace vieo;
  if (!db) return VIEO_E_INVALID;
  auto it = db->index.find(kf_id);
  if (it == db->index.end()) {
    set_error("kfdb: key frame %lld is not stored", (long long)kf_id);
    return VIEO_E_INVALID;
  }
  db->dead += db->kfs[it->second].count;
  db->kfs.erase(db->kfs.begin() + it->second);
  kfdb_reindex(db);
  if (db->dead * 2 > db->words.size()) kfdb_compact(db);
  db->last_valid = false;
  return VIEO_OK;
}

extern "C" int vieo_kfdb_set_covisible(vieo_kfdb* db, int64_t kf_id, const int64_t* ids, int n) {
  if (!db || n < 0 || n > 10 || (n > 0 && !ids)) return VIEO_E_INVALID;
  auto it = db->index.find(kf_id);
  if (it == db->index.end()) {
    vieo::set_error("kfdb: key frame %lld is not stored", (long long)kf_id);
    return VIEO_E_INVALID;
  }
  vieo::KfdbEntry& e = db->kfs[it->second];
  e.n_covis = n;
  for (int i = 0; i < n; i++) e.covis[i] = ids[i];
  return VIEO_OK;
}

extern "C" int vieo_kfdb_scores(vieo_kfdb* db, const uint32_t* word_id, const double* word_value, int n_words,
                                const int64_t* kf_ids, int n_ids, double* out) {
  using namespace vieo;
  int rc = kfdb_query_ok(db, word_id, word_value, n_words);
  if (rc != VIEO_OK) return rc;
  if (n_ids < 0 || (n_ids > 0 && (!kf_ids || !out))) return VIEO_E_INVALID;
  std::vector<int> pos(n_ids);
  for (int i = 0; i < n_ids; i++) {
    auto it = db->index.find(kf_ids[i]);
    if (it == db->index.end()) {
      set_error("kfdb: key frame %lld is not stored", (long long)kf_ids[i]);
      return VIEO_E_INVALID;
    }
    pos[i] = it->second;
  }
  std::vector<KfdbScore> sc;
  if ((rc = kfdb_run(db, word_id, word_value, n_words, pos.data(), n_ids, sc)) != VIEO_OK) return rc;
  for (int i = 0; i < n_ids; i++) out[i] = sc[i].score;
  return VIEO_OK;
}

extern "C" int vieo_kfdb_detect_reloc(vieo_kfdb* db, const uint32_t* word_id, const double* word_value, int n_words,
                                      int64_t* out_ids, int capacity, int32_t* n_out) {
  return vieo::kfdb_detect(db, word_id, word_value, n_words, false, nullptr, 0, 0.f, out_ids, capacity, n_out);
}

extern "C" int vieo_kfdb_detect_loop(vieo_kfdb* db, const uint32_t* word_id, const double* word_value, int n_words,
                                     const int64_t* connected_ids, int n_connected, float min_score, int64_t* out_ids,
                                     int capacity, int32_t* n_out) {
  return vieo::kfdb_detect(db, word_id, word_value, n_words, true, connected_ids, n_connected, min_score, out_ids, capacity,
                           n_out);
}

extern "C" int vieo_kfdb_tap_query(const vieo_kfdb* db, int64_t* kf_ids, int32_t* n_common, uint32_t* first_word,
                                   double* score) {
  if (!db) return VIEO_E_INVALID;
  if (!db->last_valid) return VIEO_E_EMPTY;
  for (size_t i = 0; i < db->last.size(); i++) {
    if (kf_ids) kf_ids[i] = db->kfs[i].id;
    if (n_common) n_common[i] = db->last[i].n_common;
    if (first_word) first_word[i] = db->last[i].first_word;
    if (score) score[i] = db->last[i].score;
  }
  return VIEO_OK;
}
