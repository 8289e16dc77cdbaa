// The host half of the PnP and Sim3 RANSAC handles (vieo_slam_amd/csrc/ransac_table.h) behind a C interface, for
// tests/test_ransac_table.py: one handle of each kind, filled from synthetic tables the way pnp.hip and sim3_solver.hip
// fill theirs from the device's.  Test only.
#include <cstdarg>
#include <cstdio>

#include "../../vieo_slam_amd/csrc/ransac_table.h"

static char g_error[512];
namespace vieo {
void set_error(const char* fmt, ...) {  // the library's keeps the text per thread; this one keeps the last
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
}
}  // namespace vieo

struct Job {  // PnpJob of pnp_device.h
  int cand, idx_off, cnt, mask_off;
};
static vieo_pnp g_pnp;
static vieo_sim3_solver g_sim3;
static std::vector<Job> g_jobs;
static std::vector<int32_t> g_idx;
static size_t g_rec_words;

template <class H, class P, class Set>
static int make(H& h, int K, const int* n, const int* n_out, const int32_t* index, const P& params, Set set_parameters, int S,
                const int32_t* samples, uint64_t seed, int* bad) {
  h = H();
  h.n_rows = S;
  h.cands.resize(K);
  for (int c = 0; c < K; index += n[c], c++) {
    h.cands[c].set(n[c], n_out[c], index);
    set_parameters(h.cands[c], params);
  }
  vieo::RansacBadSample b{-1, -1, -1};
  const bool ok = h.fill_samples(samples, seed, b);
  bad[0] = b.cand, bad[1] = b.row, bad[2] = b.index;
  return ok ? 0 : -1;
}

template <class H>
static void slice_all(H& h, const double* pose, const int32_t* count, const uint64_t* mask) {
  const vieo::RansacLayout L = h.layout();
  for (size_t c = 0; c < h.cands.size(); c++)
    if (h.cands[c].alive) h.cands[c].slice((int)c, h.n_rows, L.mask_off[c], pose, count, mask);
}

template <class H>
static void info_of(const H& h, int cand, int32_t* o) {
  const auto& Q = h.cands[cand];
  o[0] = Q.n, o[1] = Q.n_out, o[2] = Q.words, o[3] = Q.min_inliers, o[4] = Q.max_its, o[5] = Q.alive;
  o[6] = Q.iterations, o[7] = Q.best_inliers, o[8] = Q.best_row;
}

template <class H>
static void layout_of(const H& h, int* off, int* words, int* mask_off, long long* totals) {
  const vieo::RansacLayout L = h.layout();
  for (size_t c = 0; c < h.cands.size(); c++) off[c] = L.off[c], words[c] = L.words[c], mask_off[c] = L.mask_off[c];
  totals[0] = (long long)L.n_all, totals[1] = (long long)L.words_all;
}

extern "C" {

const char* rt_error() { return g_error; }
void rt_clear_error() { g_error[0] = 0; }
void rt_draw(uint64_t seed, int cand, int row, int n, int k, int32_t* out) { vieo::ransac_draw(seed, cand, row, n, k, out); }
int rt_max_iterations(double probability, float epsilon, int min_inliers, int N, int max_iterations) {
  return vieo::ransac_max_iterations(probability, epsilon, min_inliers, N, max_iterations);
}
void rt_mark_inliers(const uint64_t* mask_row, int n, const int32_t* index_map, uint8_t* out) {
  vieo::mark_inliers(mask_row, n, index_map, out);
}

// which: 0 the PnP handle, 1 the Sim3 handle
int rt_pnp_new(int K, const int* n, const int* n_out, const int32_t* index, const vieo_pnp_params* P, int S, const int32_t* samples,
               uint64_t seed, int* bad) {
  g_jobs.clear(), g_idx.clear(), g_rec_words = 0;
  return make(g_pnp, K, n, n_out, index, *P, vieo::pnp_set_ransac_parameters, S, samples, seed, bad);
}
int rt_sim3_new(int K, const int* n, const int* n_out, const int32_t* index, const vieo_sim3_params* P, int S, const int32_t* samples,
                uint64_t seed, int* bad) {
  return make(g_sim3, K, n, n_out, index, *P, vieo::sim3_set_ransac_parameters, S, samples, seed, bad);
}
void rt_layout(int which, int* off, int* words, int* mask_off, long long* totals) {
  which ? layout_of(g_sim3, off, words, mask_off, totals) : layout_of(g_pnp, off, words, mask_off, totals);
}
void rt_info(int which, int cand, int32_t* o) {
  which ? info_of(g_sim3, cand, o) : info_of(g_pnp, cand, o);
  o[9] = which ? 0 : (int32_t)g_pnp.cands[cand].rec_row.size();
}
// the downloads of all candidates: pose[K][S][12 or 13], count[K][S], mask[words_all]; for PnP the records are chosen
void rt_rows(int which, const double* pose, const int32_t* count, const uint64_t* mask) {
  if (which) return slice_all(g_sim3, pose, count, mask);
  slice_all(g_pnp, pose, count, mask);
  vieo::pnp_select_records(g_pnp, g_jobs, g_idx, g_rec_words);
}
void rt_pnp_sizes(long long* o) { o[0] = (long long)g_jobs.size(), o[1] = (long long)g_idx.size(), o[2] = (long long)g_rec_words; }
void rt_pnp_jobs(int* jobs, int32_t* idx) {
  for (size_t j = 0; j < g_jobs.size(); j++)
    jobs[4 * j] = g_jobs[j].cand, jobs[4 * j + 1] = g_jobs[j].idx_off, jobs[4 * j + 2] = g_jobs[j].cnt, jobs[4 * j + 3] = g_jobs[j].mask_off;
  for (size_t i = 0; i < g_idx.size(); i++) idx[i] = g_idx[i];
}
// pass B's downloads: Rt[n_jobs][12], count[n_jobs], mask[rec_words]
void rt_pnp_records(const double* rt, const int32_t* cnt, const uint64_t* mask) { vieo::pnp_store_records(g_pnp, g_jobs, rt, cnt, mask); }
int rt_pnp_rec_rows(int cand, int32_t* rec_row, int32_t* rec_of_row) {
  const vieo::PnpCand& Q = g_pnp.cands[cand];
  for (size_t i = 0; i < Q.rec_row.size(); i++) rec_row[i] = Q.rec_row[i];
  for (size_t i = 0; i < Q.rec_of_row.size(); i++) rec_of_row[i] = Q.rec_of_row[i];
  return (int)Q.rec_row.size();
}
int rt_iterate(int which, int cand, int n_iterations, int32_t* found, float* T, uint8_t* inliers, int32_t* n_inliers, int32_t* no_more,
               int32_t* row_used) {
  return which ? vieo::sim3_iterate(g_sim3, cand, n_iterations, found, T, inliers, n_inliers, no_more, row_used)
               : vieo::pnp_iterate(g_pnp, cand, n_iterations, found, T, inliers, n_inliers, no_more, row_used);
}
int rt_tap_rows(int which, int cand, int32_t* samples, double* pose, int32_t* count, uint64_t* mask) {
  return which ? g_sim3.tap_rows(cand, samples, pose, count, mask) : g_pnp.tap_rows(cand, samples, pose, count, mask);
}
int rt_sim3_estimate(int cand, float* R12, float* t12, float* s12) { return vieo::sim3_get_estimate(g_sim3, cand, R12, t12, s12); }

}  // extern "C"
