// ransac_table.h -- the host half of the two RANSAC handles, PnPsolver (pnp.hip) and Sim3Solver (sim3_solver.hip): the
// sample table and its draw, the tail of SetRansacParameters, where K candidates' S rows lie in the concatenated device
// tables, one candidate's row table (pose[S][D], count[S], mask[S][words]), and the two replays of iterate over such
// tables, which hold the reference's order-dependent bookkeeping.  Host-only C++ (no HIP): the tests compile it with
// g++ (tests/emul/ransac_table_emul.cc, tests/test_ransac_table.py).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/vieo_hot.h"

namespace vieo {

void set_error(const char* fmt, ...);

// the library's own draw when the caller passes no table: a counter-based generator (splitmix64 of seed, candidate,
// row, draw), k indices without replacement in the reference's swap-with-back manner (PnPsolver.cc:174-186,
// Sim3Solver.cc:164-178)
inline uint64_t ransac_mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
inline void ransac_draw(uint64_t seed, int cand, int row, int n, int k, int32_t* out) {
  std::vector<int32_t> avail(n);
  for (int i = 0; i < n; i++) avail[i] = i;
  for (int i = 0; i < k; i++) {
    const uint64_t r = ransac_mix(ransac_mix(seed ^ ((uint64_t)cand << 40)) + ((uint64_t)row << 2) + i);
    const int j = (int)(r % (uint64_t)avail.size());
    out[i] = avail[j];
    avail[j] = avail.back();
    avail.pop_back();
  }
}

// the tail of SetRansacParameters (PnPsolver.cc:133-147, Sim3Solver.cc:127-141): mRansacMaxIts from the epsilon the
// solver has settled on
inline int ransac_max_iterations(double probability, float epsilon, int min_inliers, int N, int max_iterations) {
  if (min_inliers == N) return 1;
  const double its = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)epsilon, 3.0)));
  const int nIterations = !(its < 2147483647.0) ? 2147483647 : its < 1.0 ? 1 : (int)its;  // (a NaN ends as the cap below)
  return std::max(1, std::min(nIterations, max_iterations));
}

inline bool mask_bit(const uint64_t* mask_row, int i) { return (mask_row[i / 64] >> (i % 64)) & 1; }
// the correspondences of a mask row, ascending, appended to idx
inline void mask_indices(const uint64_t* mask_row, int n, std::vector<int32_t>& idx) {
  for (int i = 0; i < n; i++)
    if (mask_bit(mask_row, i)) idx.push_back(i);
}
// vbInliers[index_map[i]] = true for every correspondence of a mask row
inline void mark_inliers(const uint64_t* mask_row, int n, const int32_t* index_map, uint8_t* out) {
  for (int i = 0; i < n; i++)
    if (mask_bit(mask_row, i)) out[index_map[i]] = 1;
}

// [s R | t] of a pose row as floats in a 4 x 4 identity: Rcw / tcw .convertTo(CV_32F) with s = 1 (PnPsolver.cc:200-206,
// :264-270; the product by 1 is exact), mBestT12 with the row's scale (Sim3Solver.cc:199)
inline void pose_float(const double* Rt, double s, float* T) {
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) T[4 * r + c] = (float)(s * Rt[3 * r + c]);
    T[4 * r + 3] = (float)Rt[9 + r];
  }
  T[12] = T[13] = T[14] = 0.f, T[15] = 1.f;
}

// one candidate: its rows of the hypothesis table and the solver's state between iterate calls.  D doubles per pose.
template <int D>
struct RansacRows {
  static const int kPose = D;
  int n = 0, n_out = 0, words = 0;  // correspondences; the length of vbInliers (n_frame_keys, n1); words of a mask row
  int min_inliers = 0, max_its = 1;
  bool alive = false;          // N >= mRansacMinInliers: the candidate has a solver
  std::vector<int32_t> index;  // [n] correspondence -> entry of vbInliers (mvKeyPointIndices, mvnIndices1)
  std::vector<double> pose;    // [n_rows][D]
  std::vector<int32_t> count;  // [n_rows]
  std::vector<uint64_t> mask;  // [n_rows][words]
  int iterations = 0, best_inliers = 0, best_row = -1;

  void set(int n_, int n_out_, const int32_t* index_) {
    n = n_, n_out = n_out_, words = (n_ + 63) / 64, index.assign(index_, index_ + n_);
  }
  // candidate c's S rows out of the downloads of all candidates
  void slice(int c, int S, size_t mask_off, const double* pose_all, const int32_t* count_all, const uint64_t* mask_all) {
    pose.assign(pose_all + (size_t)c * S * D, pose_all + (size_t)(c + 1) * S * D);
    count.assign(count_all + (size_t)c * S, count_all + (size_t)(c + 1) * S);
    mask.assign(mask_all + mask_off, mask_all + mask_off + (size_t)S * words);
  }
  const double* pose_row(int r) const { return &pose[(size_t)r * D]; }
  const uint64_t* mask_row(int r) const { return &mask[(size_t)r * words]; }
};

struct RansacBadSample { int cand, row, index; };
struct RansacLayout {  // per candidate: its first correspondence, the words of a mask row (0: no solver), its first mask word
  std::vector<int> off, words, mask_off;
  size_t n_all = 0, words_all = 0;
};

// the handle: K candidates and their sample rows of SET indices
template <class Cand, int SET>
struct RansacTable {
  std::vector<Cand> cands;
  std::vector<int32_t> samples;  // [K][n_rows][SET]; the rows of a candidate without a solver stay 0
  int n_rows = 0;

  bool has(int cand) const { return cand >= 0 && cand < (int)cands.size(); }
  // the caller's table src[K][n_rows][SET] after its check (every index in range and not drawn twice in its row), or
  // the library's draw; false: bad names the first offence
  bool fill_samples(const int32_t* src, uint64_t seed, RansacBadSample& bad) {
    samples.assign(cands.size() * n_rows * SET, 0);
    for (int c = 0; c < (int)cands.size(); c++) {
      if (!cands[c].alive) continue;
      for (int r = 0; r < n_rows; r++) {
        const size_t at = ((size_t)c * n_rows + r) * SET;
        if (!src) ransac_draw(seed, c, r, cands[c].n, SET, &samples[at]);
        for (int i = 0; src && i < SET; i++) {
          bool ok = src[at + i] >= 0 && src[at + i] < cands[c].n;
          for (int j = 0; ok && j < i; j++) ok = src[at + j] != src[at + i];
          if (!ok) {
            bad = RansacBadSample{c, r, src[at + i]};
            return false;
          }
          samples[at + i] = src[at + i];
        }
      }
    }
    return true;
  }
  RansacLayout layout() const {
    RansacLayout L;
    for (const Cand& Q : cands) {
      L.off.push_back((int)L.n_all), L.words.push_back(Q.alive ? Q.words : 0), L.mask_off.push_back((int)L.words_all);
      L.n_all += Q.n;
      if (Q.alive) L.words_all += (size_t)n_rows * Q.words;
    }
    return L;
  }
  // the *_tap_rows entries (any pointer may be null); a candidate without a solver has rows of zeros
  int tap_rows(int cand, int32_t* smp, double* pose, int32_t* count, uint64_t* mask) const {
    const Cand& Q = cands[cand];
    const size_t S = n_rows, D = Cand::kPose;
    if (smp) memcpy(smp, &samples[(size_t)cand * S * SET], S * SET * 4);
    if (pose) Q.alive ? memcpy(pose, Q.pose.data(), S * D * 8) : memset(pose, 0, S * D * 8);
    if (count) Q.alive ? memcpy(count, Q.count.data(), S * 4) : memset(count, 0, S * 4);
    if (mask) Q.alive ? memcpy(mask, Q.mask.data(), S * Q.words * 8) : memset(mask, 0, S * Q.words * 8);
    return VIEO_OK;
  }
};

struct PnpCand : RansacRows<12> {  // pass A: R row-major, then t
  std::vector<int32_t> rec_of_row;          // [n_rows] the record a row opens, -1 none
  std::vector<int32_t> rec_row, rec_count;  // pass B tables [n_records]: the row that opened the record, ...
  std::vector<double> rec_Rt, usun;         // ...; usun [n][2], handles of vieo_pnp_create_rig (test tap)
  std::vector<uint64_t> rec_mask;
  int best_rec = -1;
};

using Sim3Cand = RansacRows<13>;  // R row-major, t, s

}  // namespace vieo

struct vieo_pnp : vieo::RansacTable<vieo::PnpCand, 4> { bool rig = false; };
struct vieo_sim3_solver : vieo::RansacTable<vieo::Sim3Cand, 3> {};

namespace vieo {

// ---- PnPsolver
// SetRansacParameters (PnPsolver.cc:115-147) of a candidate of N = Q.n correspondences, and whether it has a solver
inline void pnp_set_ransac_parameters(PnpCand& Q, const vieo_pnp_params& P) {
  const int N = Q.n;
  if (N > 0) {
    float epsilon = P.epsilon;
    int nMinInliers = (int)((float)N * epsilon);
    if (nMinInliers < P.min_inliers) nMinInliers = P.min_inliers;
    if (nMinInliers < P.min_set) nMinInliers = P.min_set;
    Q.min_inliers = nMinInliers;
    if (epsilon < (float)Q.min_inliers / N) epsilon = (float)Q.min_inliers / N;
    Q.max_its = ransac_max_iterations(P.probability, epsilon, Q.min_inliers, N, P.max_iterations);
  }
  Q.alive = N >= 4 && N >= Q.min_inliers;
  if (N > 0 && N < 4) Q.min_inliers = std::max(Q.min_inliers, 4);  // N < mRansacMinInliers: bNoMore at once
  if (N == 0) Q.min_inliers = std::max(P.min_inliers, 4), Q.max_its = 1;
}

// the records: the rows that raise the best-so-far set (PnPsolver.cc:194-199), in candidate then row order.  Per
// record a pass-B job {candidate, first index, count, first mask word} and the indices of its inliers in idx.
template <class Job>
inline void pnp_select_records(vieo_pnp& H, std::vector<Job>& jobs, std::vector<int32_t>& idx, size_t& rec_words) {
  rec_words = 0;
  for (int c = 0; c < (int)H.cands.size(); c++) {
    PnpCand& Q = H.cands[c];
    if (!Q.alive) continue;
    Q.rec_of_row.assign(H.n_rows, -1);
    int best = 0;
    for (int r = 0; r < H.n_rows; r++) {
      if (Q.count[r] < Q.min_inliers || Q.count[r] <= best) continue;
      best = Q.count[r];
      Q.rec_of_row[r] = (int)Q.rec_row.size();
      Q.rec_row.push_back(r);
      jobs.push_back(Job{c, (int)idx.size(), Q.count[r], (int)rec_words});
      mask_indices(Q.mask_row(r), Q.n, idx);
      rec_words += Q.words;
    }
  }
}

// pass B's downloads, one row per job, to their candidates
template <class Job>
inline void pnp_store_records(vieo_pnp& H, const std::vector<Job>& jobs, const double* rt, const int32_t* cnt, const uint64_t* mask) {
  for (size_t j = 0; j < jobs.size(); j++) {
    PnpCand& Q = H.cands[jobs[j].cand];
    Q.rec_Rt.insert(Q.rec_Rt.end(), rt + j * 12, rt + (j + 1) * 12);
    Q.rec_count.push_back(cnt[j]);
    Q.rec_mask.insert(Q.rec_mask.end(), mask + jobs[j].mask_off, mask + jobs[j].mask_off + Q.words);
  }
}

// PnPsolver::iterate (PnPsolver.cc:154-233) over the two tables; the arguments are vieo_pnp_iterate's, checked there
inline int pnp_iterate(vieo_pnp& H, int cand, int n_iterations, int32_t* found, float* Tcw, uint8_t* inliers,
                       int32_t* n_inliers, int32_t* no_more, int32_t* row_used) {
  PnpCand& Q = H.cands[cand];
  *found = 0, *n_inliers = 0, *no_more = 0;
  if (row_used) *row_used = -1;
  if (Q.n_out > 0) memset(inliers, 0, Q.n_out);  // vbInliers.clear()
  if (Q.n < Q.min_inliers || !Q.alive) {
    *no_more = 1;
    return VIEO_OK;
  }
  auto give = [&](const double* Rt, const uint64_t* mask, int count, int row) {
    *found = 1, *n_inliers = count;
    if (row_used) *row_used = row;
    pose_float(Rt, 1.0, Tcw);
    memset(inliers, 0, Q.n_out);
    mark_inliers(mask, Q.n, Q.index.data(), inliers);
  };
  int current = 0;
  while (Q.iterations < Q.max_its || current < n_iterations) {
    if (Q.iterations >= H.n_rows) {
      set_error("PnPsolver: candidate %d needs sample row %d, the table has %d", cand, Q.iterations, H.n_rows);
      return VIEO_E_CAPACITY;
    }
    const int row = Q.iterations;
    current++, Q.iterations++;
    if (Q.count[row] < Q.min_inliers) continue;
    if (Q.count[row] > Q.best_inliers) Q.best_inliers = Q.count[row], Q.best_row = row, Q.best_rec = Q.rec_of_row[row];
    const int rec = Q.best_rec;  // Refine works on the best-so-far set, whichever row opened it
    if (Q.rec_count[rec] > Q.min_inliers) {
      give(&Q.rec_Rt[(size_t)rec * 12], &Q.rec_mask[(size_t)rec * Q.words], Q.rec_count[rec], row);
      return VIEO_OK;
    }
  }
  if (Q.iterations >= Q.max_its) {
    *no_more = 1;
    if (Q.best_inliers >= Q.min_inliers) give(Q.pose_row(Q.best_row), Q.mask_row(Q.best_row), Q.best_inliers, Q.best_row);
  }
  return VIEO_OK;
}

// ---- Sim3Solver
// SetRansacParameters (Sim3Solver.cc:118-141); a candidate below minInliers has no solver and keeps max_its 1
inline void sim3_set_ransac_parameters(Sim3Cand& Q, const vieo_sim3_params& P) {
  Q.min_inliers = P.min_inliers;
  Q.alive = Q.n >= Q.min_inliers;  // (min_inliers >= 3: a solver has its 3 points)
  if (Q.alive) Q.max_its = ransac_max_iterations(P.probability, (float)P.min_inliers / Q.n, P.min_inliers, Q.n, P.max_iterations);
}

// Sim3Solver::iterate (Sim3Solver.cc:143-219) over the table; the arguments are vieo_sim3_iterate's, checked there
inline int sim3_iterate(vieo_sim3_solver& H, int cand, int n_iterations, int32_t* found, float* T12, uint8_t* inliers,
                        int32_t* n_inliers, int32_t* no_more, int32_t* row_used) {
  Sim3Cand& Q = H.cands[cand];
  *found = 0, *n_inliers = 0, *no_more = 0;
  if (row_used) *row_used = -1;
  if (Q.n_out > 0) memset(inliers, 0, Q.n_out);  // vbInliers = vector<bool>(mN1, false)
  if (!Q.alive) {  // N < mRansacMinInliers
    *no_more = 1;
    return VIEO_OK;
  }
  int current = 0;
  while (Q.iterations < Q.max_its && current < n_iterations) {
    if (Q.iterations >= H.n_rows) {
      set_error("Sim3Solver: candidate %d needs sample row %d, the table has %d", cand, Q.iterations, H.n_rows);
      return VIEO_E_CAPACITY;
    }
    const int row = Q.iterations;
    current++, Q.iterations++;
    if (Q.count[row] < Q.best_inliers) continue;
    Q.best_inliers = Q.count[row], Q.best_row = row;
    if (Q.count[row] > Q.min_inliers) {
      pose_float(Q.pose_row(row), Q.pose_row(row)[12], T12);
      mark_inliers(Q.mask_row(row), Q.n, Q.index.data(), inliers);
      *found = 1, *n_inliers = Q.count[row];
      if (row_used) *row_used = row;
      return VIEO_OK;
    }
  }
  if (Q.iterations >= Q.max_its) *no_more = 1;
  return VIEO_OK;
}

// GetEstimatedRotation / Translation / Scale: mBestRotation, mBestTranslation, mBestScale as floats
inline int sim3_get_estimate(const vieo_sim3_solver& H, int cand, float* R12, float* t12, float* s12) {
  const Sim3Cand& Q = H.cands[cand];
  if (Q.best_row < 0) {
    set_error("Sim3Solver: candidate %d has no estimate yet", cand);
    return VIEO_E_EMPTY;
  }
  const double* o = Q.pose_row(Q.best_row);
  for (int i = 0; i < 9; i++) R12[i] = (float)o[i];
  for (int i = 0; i < 3; i++) t12[i] = (float)o[9 + i];
  *s12 = (float)o[12];
  return VIEO_OK;
}

}  // namespace vieo
