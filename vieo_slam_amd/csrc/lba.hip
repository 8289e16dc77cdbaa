// lba.hip -- Optimizer::LocalBundleAdjustment on gfx950 (reference: src/Optimizer.cc:1876-2307;
// g2o BlockSolver<6,3> with Schur complement, block_solver.hpp:353-589; LM
// optimization_algorithm_levenberg.cpp:61-207; edges src/Odom/g2otypes.h:321-547).
//
// Several independent windows advance in lock step; every kernel covers all windows of the batch
// (grid y / x = window) and returns at once for windows whose control word does not ask for the step.
// Device side (all FP64, no floating-point atomics: every sum has a fixed order, so a window's result
// does not depend on what it is batched with), one header per stage; each opens with its kernels, their grids and LDS,
// the LbaDev fields they read and write and who launches them:
//   lba_device.h             LbaKf / LbaImu / LbaDev, the accessors, the visual edge's residual and Jacobians
//   lba_inertial_device.h    the inertial / encoder pair edges: lba_generic_dev, k_lba_generic
//   lba_state_device.h       k_lba_restore / classify / prelevel / zero / begin / error / reduce, k_lba_update_points,
//                            k_lba_tail
//   lba_linearize_device.h   k_lba_build and its folds, k_lba_lambda
//   lba_schur_device.h       k_lba_occ, k_lba_schur, k_lba_pack, the reduced system's entries, k_lba_assemble[_tiles]
//   lba_solve_device.h       lba_apply_step, k_lba_ldlt16, k_lba_ldltg, k_big_* and their launch contract
// This file is the host side: the call record and its checks, the arena layout and staging, the lock-step round
// (launch_round, launch_big_ldlt), landmark sharding, the kernel-class timers and the C-ABI.  Nothing below the
// `host-side` divider is visible to the headers.
// The Levenberg-Marquardt policy (lambda, accept / reject, termination, stop flag) runs on the host
// exactly as g2o's does, from one WinOut record per window and round (lba_policy.h).
#include <atomic>
#include <chrono>
#include <mutex>
#include <thread>
#include <vector>

#include "gba_sparse_plan.h"
#include "lba_policy.h"
#include "rccl_dl.h"

// the device side, in the order of a round
#include "lba_device.h"
#include "lba_inertial_device.h"
#include "lba_state_device.h"
#include "lba_linearize_device.h"
#include "lba_schur_device.h"
#include "lba_solve_device.h"

namespace vieo {

// ================================================================== host-side lock-step LM driver
static thread_local hipStream_t g_lba_stream = nullptr;
static thread_local int g_lba_stream_dev = -1;  // the device the stream was created on
static thread_local int g_lba_priority = -2;    // vieo_lba_set_stream_priority of this host thread (-2: VIEO_LBA_PRIORITY / -1)
static thread_local DevBuf g_arena, g_small;
static thread_local PinnedBuf g_stage, g_small_h;

struct WinHost {  // a window of a call on the host
  const vieo_lba_params* P;
  const vieo_lba_vio_params* VP = nullptr;  // visual-inertial window (a18)
  const vieo_lba_enc* ENC = nullptr;        // encoder edges of a vision-only window (a17)
  int n_kf, n_mp, n_obs, n_imu = 0;
  int nf = 0;  // free key frames
  bool skip = false;   // takes no part in the rounds: no free pose, or the stop flag was up at entry
  int cls = 0;         // solver_class of its reduced system
  GbaSparsePlan plan;  // class 3: the symbolic plan of the tile-sparse solve
  WinLm lm;            // its LM state machine (lba_policy.h)
  size_t o_kf, o_X, o_erase, o_scl;  // offsets of the results in the staging buffer (plan_window)
};

// n x n inverse (n <= 9) by Gauss-Jordan with partial pivoting: the 9 x 9 pre-integration covariance
// (GetProcessedInfoijPRV: mSigmaijPRV.inverse()), the 6 x 6 encoder covariance
static bool inverse_n(const double* A, double* Ainv, int n) {
  double M[9][18];
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) M[i][j] = A[i * n + j], M[i][n + j] = (i == j);
  for (int c = 0; c < n; c++) {
    int piv = c;
    for (int r = c + 1; r < n; r++)
      if (std::fabs(M[r][c]) > std::fabs(M[piv][c])) piv = r;
    if (M[piv][c] == 0) return false;
    if (piv != c)
      for (int j = 0; j < 2 * n; j++) std::swap(M[c][j], M[piv][j]);
    const double d = M[c][c];
    for (int j = 0; j < 2 * n; j++) M[c][j] /= d;
    for (int r = 0; r < n; r++)
      if (r != c) {
        const double f = M[r][c];
        if (f != 0)
          for (int j = 0; j < 2 * n; j++) M[r][j] -= f * M[c][j];
      }
  }
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) Ainv[i * n + j] = M[i][n + j];
  return true;
}

struct LbaShard {  // landmark-sharded run: every rank holds all key frames and its share of the points
  vieo_allreduce_sum_f64_fn fn;
  void* ctx;
  double* d_buf;
  size_t cap;
};

// one exchange of a sharded run: the caller's callback (complete on return; the stream is drained first) or, with
// fn == nullptr, ncclAllReduce on the stream itself (ctx = the communicator of vieo_rccl_comm_create)
static int shard_exchange(const LbaShard* sh, double* d_buf, size_t n, hipStream_t st) {
  if (sh->fn) {
    VIEO_HIP_CHECK(hipStreamSynchronize(st));
    if (sh->fn(sh->ctx, d_buf, n) != 0) {
      set_error("sharded local BA: the all-reduce callback failed");
      return VIEO_E_INVALID;
    }
    return VIEO_OK;
  }
  return rccl_allreduce_sum_f64(sh->ctx, d_buf, n, st);
}

// All ranks of a sharded run agree on go / no-go: the sum of the ranks' failure flags through the run's own exchange.
// Every rank must call it the same number of times.  *sum > 0: some rank failed.
// stop / *stop_any: the ranks' stop requests travel in the same number (4096 per request: exact in a double for any
// realistic job size), so that pbStopFlag raised on one rank aborts the call on all of them together.
static int shard_agree(const LbaShard* sh, bool ok, double* sum, bool stop = false, bool* stop_any = nullptr) {
  const double flag = (ok ? 0.0 : 1.0) + (stop ? 4096.0 : 0.0);
  *sum = 1.0;
  VIEO_HIP_CHECK(hipMemcpy(sh->d_buf, &flag, 8, hipMemcpyHostToDevice));
  const int xrc = shard_exchange(sh, sh->d_buf, 1, nullptr);
  if (xrc != VIEO_OK) return xrc;
  VIEO_HIP_CHECK(hipStreamSynchronize(nullptr));
  double total = 0;
  VIEO_HIP_CHECK(hipMemcpy(&total, sh->d_buf, 8, hipMemcpyDeviceToHost));
  const double stops = std::floor(total / 4096.0);
  if (stop_any) *stop_any = stops > 0;
  *sum = total - 4096.0 * stops;
  return VIEO_OK;
}

// A rank that leaves lba_run between the first agreement and the rounds (a staging error only it ran into: allocation
// failure, a singular covariance) still takes part in the second agreement -- with a failure flag -- so that the
// other ranks return too instead of waiting for it in the first all-reduce of the rounds.
struct ShardStagingGuard {
  const LbaShard* sh;
  bool done = false;
  ~ShardStagingGuard() {
    if (sh && !done) {
      double sum;
      (void)shard_agree(sh, false, &sum);
    }
  }
};

// packed reduced visual system of a window with nf free key frames (k_lba_pack); sc: with the scale vertex's row,
// H_ps, H_ss, b_s
static size_t shard_sys_doubles(int nf, int sc = 0) {
  const size_t nv = (size_t)6 * nf + (sc ? 1 : 0);
  return nv * (nv + 1) + 36 * (size_t)nf + 6 * (size_t)nf + (sc ? 6 * (size_t)nf + 2 : 0);
}

// reduced systems beyond one workgroup's LDL^T take the tiled solve (VIEO_LBA_BIG_SOLVE=1 forces it: tests)
static const int kSmallSolveMax = 16 * kLdGMaxBlocks - 1, kBigSolveMax = 16320;
// ---- optional kernel-class timing (vieo_lba_enable_timing): HIP events around every launch on the BA stream, folded
// into process-wide totals after each round's synchronisation.  bench.py reads them for the roofline of the whole path.
enum LbaKClass { KC_BUILD, KC_GENERIC, KC_SCHUR, KC_ASSEMBLE, KC_LDLT, KC_UPDATE, KC_ERROR, KC_BEGIN, KC_OTHER, KC_LDLT_SPARSE, KC_N };
static const char* const kLbaKClassName[KC_N] = {"lba.build", "lba.generic", "lba.schur", "lba.assemble", "lba.ldlt",
                                                 "lba.update_points", "lba.error", "lba.begin", "lba.other",
                                                 "lba.ldlt_sparse"};
static std::atomic<int> g_lba_ktiming{0};
static std::mutex g_lba_kt_mutex;
static double g_lba_kt_ms[KC_N];
static long long g_lba_kt_launches[KC_N];
static double g_lba_kt_schur_flops;  // dense FLOPs of the timed k_lba_schur launches
// the last tile-sparse call of this process (vieo_lba_sparse_stats): stored tiles, tiles of the dense lower triangle,
// planned Schur tiles, planned upper Schur tiles of the dense grid, plan bytes, arena bytes
static long long g_lba_sparse_stats[6];

struct LbaKTimer {
  bool on = false, count_only = false;  // count_only (mode 2): launches per class without events
  hipStream_t st = nullptr;
  std::vector<hipEvent_t> pool;
  std::vector<int> cls;  // class of pair i (events 2i, 2i + 1)
  void begin(hipStream_t s) {
    const int mode = g_lba_ktiming.load();
    on = mode != 0, count_only = mode == 2;
    st = s;
    cls.clear();
  }
  template <class F>
  void launch(int c, F&& f) {
    if (!on) {
      f();
      return;
    }
    if (count_only) {
      f();
      cls.push_back(c);
      return;
    }
    const size_t i = cls.size();
    while (pool.size() < 2 * (i + 1)) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) {
        on = false;
        f();
        return;
      }
      pool.push_back(e);
    }
    (void)hipEventRecord(pool[2 * i], st);
    f();
    (void)hipEventRecord(pool[2 * i + 1], st);
    cls.push_back(c);
  }
  void fold(double schur_flops_per_launch) {  // after the stream was synchronised
    if (!on || cls.empty()) return;
    std::lock_guard<std::mutex> g(g_lba_kt_mutex);
    bool schur_seen = false;  // a round's Schur complement is two launches (diagonal / off-diagonal tiles): FLOPs once
    for (size_t i = 0; i < cls.size(); i++) {
      float ms = 0;
      if (!count_only && hipEventElapsedTime(&ms, pool[2 * i], pool[2 * i + 1]) != hipSuccess) continue;
      g_lba_kt_ms[cls[i]] += ms, g_lba_kt_launches[cls[i]]++;
      if (cls[i] == KC_SCHUR && !schur_seen) g_lba_kt_schur_flops += schur_flops_per_launch, schur_seen = true;
    }
    cls.clear();
  }
};

static bool big_solve(int n) {
  static const int forced = [] {
    const char* e = getenv("VIEO_LBA_BIG_SOLVE");
    return e ? atoi(e) : 0;
  }();
  return forced > 0 || n > kSmallSolveMax;
}

static bool sparse_solve_forced() {  // VIEO_LBA_SPARSE_SOLVE=1: every full BA takes the tile-sparse solve (tests)
  static const int forced = [] {
    const char* e = getenv("VIEO_LBA_SPARSE_SOLVE");
    return e ? atoi(e) : 0;
  }();
  return forced > 0;
}

// The solve kernel of a window with n unknowns.  Windows of different classes share a lock-step batch: every class's
// kernel is launched (when one of its windows takes a trial this round) and skips the others' windows (a bLarge
// window of 25 key frames next to ordinary ones of 10 is the usual LocalMapping mix).
//   0  k_lba_ldlt16   n <= 159: blocked on the matrix cores, whole triangle in LDS
//   1  k_lba_ldltg    n <= 639: one workgroup, left-looking, the factor in L2 as column-major 16 x 16 blocks
//   2  k_big_*        the tiled LDL^T over many workgroups (full BA: hundreds of key frames)
//   3  k_big_*<TILES> the same over the stored tiles of the symbolic fill pattern (gba_sparse_plan.h): the full BA
//                     (full_ba: not landmark-sharded) beyond kBigSolveMax unknowns, or any with VIEO_LBA_SPARSE_SOLVE=1
static int solver_class(int n, bool full_ba = false) {
  if (full_ba && (sparse_solve_forced() || n > kBigSolveMax)) return 3;
  if (big_solve(n)) return 2;
  if (((n + 16) >> 4) <= kLd16MaxBlocks) return 0;
  return 1;
}

// Optimizer::BundleAdjustment / GlobalBundleAdjustmentNavStatePRV (Optimizer.cc:1353-1609, 771-1345) on the same
// engine: ONE optimize(iterations), Huber kernels on every edge iff `robust`, no chi2 classification, no
// Chi2LargeSetLevel, g2o's own initial lambda, no divergence guard.
struct GbaMode {
  int iterations, robust;
  int scale_opt = 0;          // bScaleOpt (System::FinalGBA): VertexScale + EdgeReprojectPRS[Stereo]
  double* scale_out = nullptr;  // the recovered scale (1 when the call returns early)
};

// Observation i of a window: sorted by map point, key-frame, camera and map-point indices in range, distorted
// observations monocular (nc: the window's n_cams).
static bool lba_obs_ok(const vieo_lba_obs* ob, int i, int n_mp, int n_kf, int nc) {
  const int kfi = ob[i].kf & 0xFFFFFF, ci = (ob[i].kf >> 24) & 15;
  return !(ob[i].mp < 0 || ob[i].mp >= n_mp || ob[i].kf < 0 || kfi >= n_kf || (i > 0 && ob[i].mp < ob[i - 1].mp) ||
           (nc == 0 ? ci != 0 : (ci >= nc || ob[i].ur >= 0)));
}
static int lba_obs_invalid() {
  set_error("vieo_local_bundle_adjustment: observations must be sorted by map point, key frame and camera indices in "
            "range, distorted observations monocular");
  return VIEO_E_INVALID;
}


// One call of the engine, as every bundle-adjustment entry of the C-ABI states it.  vparams == nullptr ->
// Optimizer::LocalBundleAdjustment (params, encs), otherwise LocalBundleAdjustmentNavStatePRV (vparams, h_close, h_imu,
// n_imu).  gba != nullptr: the full BA of the same kind.  sh != nullptr: this process is one rank of a landmark-sharded
// run.
struct LbaCall {
  const LbaShard* sh = nullptr;
  const GbaMode* gba = nullptr;
  int W = 0;  // windows
  const vieo_lba_params* const* params = nullptr;
  const vieo_lba_vio_params* const* vparams = nullptr;
  const vieo_lba_keyframe* const* h_kfs = nullptr;
  const float* const* h_points = nullptr;
  const uint8_t* const* h_close = nullptr;
  const vieo_lba_obs* const* h_obs = nullptr;
  const vieo_lba_imu_edge* const* h_imu = nullptr;
  const int *n_kf = nullptr, *n_mp = nullptr, *n_obs = nullptr, *n_imu = nullptr;  // per window
  volatile const int* stop = nullptr;
  vieo_navstate* const* h_navs_out = nullptr;
  float* const* h_points_out = nullptr;
  uint8_t* const* h_erase = nullptr;
  vieo_lba_result* h_results = nullptr;
  const vieo_lba_enc* const* encs = nullptr;  // EdgeEncNavStatePR of vision-only windows (Optimizer.cc:2008-2042, 1401-1438)

  bool vio() const { return vparams != nullptr; }
  int pd() const { return vio() ? 15 : 6; }  // reduced-system dims per free key frame
  int sco() const { return gba && gba->scale_opt ? 1 : 0; }
  bool stop_raised() const { return stop && *stop; }
  LmMode lm_mode() const { return LmMode{gba != nullptr, gba && gba->robust != 0, vio() && !gba}; }
};

// The argument checks of lba_run, without side effects: VIEO_OK or the error code, with its text.  A landmark-sharded
// run calls it first and lets all ranks agree on the outcome with one all-reduce: a rank that returned early on its own
// while the others were already waiting in the collective would hang them.  A rank of a sharded run may own no point
// (or no observation) of a window.  The observations of an unsharded call are checked while the staging threads copy
// them (fill_window): a pass of its own over them, on one thread, cost 0.3 ms per bench step.
static int lba_check_args(const LbaCall& c) {
  const bool vio = c.vio(), sharded = c.sh != nullptr;
  const int pd = c.pd(), sco = c.sco();
  if (c.W <= 0 || (!vio && !c.params) || !c.h_kfs || !c.n_kf || !c.h_points || !c.n_mp || !c.h_obs || !c.n_obs ||
      !c.h_navs_out || !c.h_points_out || !c.h_erase || !c.h_results || (vio && (!c.h_close || !c.h_imu || !c.n_imu))) {
    set_error("bundle adjustment: a missing argument or no window");
    return VIEO_E_INVALID;
  }
  for (int w = 0; w < c.W; w++) {
    const vieo_lba_params* P = vio ? (c.vparams[w] ? &c.vparams[w]->base : nullptr) : c.params[w];
    const vieo_lba_enc* enc = !vio && c.encs ? c.encs[w] : nullptr;
    const int n_kf = c.n_kf[w], n_mp = c.n_mp[w], n_obs = c.n_obs[w];
    if (!P || !c.h_kfs[w] || n_kf <= 0 || n_mp < 0 || n_obs < 0 || !c.h_navs_out[w] ||
        (!sharded && (n_mp == 0 || n_obs == 0)) || (n_mp > 0 && (!c.h_points[w] || !c.h_points_out[w])) ||
        (n_obs > 0 && (!c.h_obs[w] || !c.h_erase[w])) ||
        (vio && ((!c.h_close[w] && !c.gba) || c.n_imu[w] < 0 || (c.n_imu[w] > 0 && !c.h_imu[w]))) ||
        (enc && (enc->n_edges < 0 || (enc->n_edges > 0 && !enc->edges)))) {
      set_error("bundle adjustment: window %d has a missing buffer or a bad count", w);
      return VIEO_E_INVALID;
    }
    int nf = 0;
    for (int k = 0; k < n_kf; k++) nf += !c.h_kfs[w][k].fixed;
    // (the full BA's tile-sparse solve has no such limit: its device memory is checked once the arena is laid out)
    if (((!c.gba || sharded) && pd * nf + sco > kBigSolveMax) || n_kf >= (1 << 24)) {
      set_error("bundle adjustment: %d free key frames exceed the reduced-system limit of %d unknowns", nf, kBigSolveMax);
      return VIEO_E_CAPACITY;
    }
    const int ne = vio ? c.n_imu[w] : enc ? enc->n_edges : 0;
    std::vector<char> in(n_kf, 0), outk(n_kf, 0);
    for (int t = 0; t < ne; t++) {  // a chain: at most one pre-integration into and one out of every key frame
      const int a = vio ? c.h_imu[w][t].kf_i : enc->edges[t].kf_i, b = vio ? c.h_imu[w][t].kf_j : enc->edges[t].kf_j;
      if (a < 0 || a >= n_kf || b < 0 || b >= n_kf || a == b || outk[a] || in[b]) {
        set_error("local BA: the inertial / encoder edges must chain the key frames");
        return VIEO_E_INVALID;
      }
      outk[a] = 1, in[b] = 1;
    }
    const int nc = P->n_cams;
    if (nc < 0 || nc > 4 || (nc > 0 && !P->cams)) {
      set_error("local BA: n_cams must be 0..4");
      return VIEO_E_INVALID;
    }
    for (int ci = 0; ci < nc; ci++) {
      const vieo_camera& cam = P->cams[ci];
      if (cam.model < 0 || cam.model > 2 || (cam.model == VIEO_CAM_RADTAN && (cam.num_k < 2 || cam.num_k > 6))) {
        set_error("local BA: camera %d has an unknown model or coefficient count", ci);
        return VIEO_E_INVALID;
      }
    }
    for (int i = 0; sharded && i < n_obs; i++)
      if (!lba_obs_ok(c.h_obs[w], i, n_mp, n_kf, nc)) return lba_obs_invalid();
  }
  return VIEO_OK;
}

// Check the call; the ranks of a sharded run agree on the outcome (first agreement) and on the stop flag.
// (configuration errors, the same on every rank of a job; `stop` is rank-local and asynchronous: a sharded run never
// acts on its own copy -- the ranks' requests are summed in the exchanges the run makes anyway (the two agreements
// at entry, the fourth scalar of every trial), so all ranks take the abort at the same point: Optimizer.cc:524-528,570-571)
static int lba_check_and_agree(const LbaCall& c, bool* shard_stop) {
  const LbaShard* sh = c.sh;
  if (sh && (!c.vio() || (!sh->fn && !sh->ctx) || !sh->d_buf)) {
    set_error("sharded local BA: visual-inertial windows only, with a reduction callback and buffer");
    return VIEO_E_INVALID;
  }
  const int rc = require_device();  // (a rank without a device cannot take part in the job at all)
  if (rc != VIEO_OK) return rc;
  if (!sh) return lba_check_args(c);
  // every rank reaches this collective whatever its own arguments look like; the sum of the failure flags decides
  // for all of them
  const bool ok = sh->cap >= 1 && lba_check_args(c) == VIEO_OK;
  double sum = 1.0;
  if (sh->cap >= 1) {
    const int xrc = shard_agree(sh, ok, &sum, c.stop_raised(), shard_stop);
    if (xrc != VIEO_OK) return xrc;
  }
  if (sum != 0.0) {
    set_error(ok ? "sharded local BA: another rank rejected its arguments, all ranks return"
                 : "sharded local BA: invalid arguments on this rank (all ranks return)");
    return VIEO_E_INVALID;
  }
  return VIEO_OK;
}

// This host thread's bundle-adjustment stream on the current device.
static int lba_stream(hipStream_t* st) {
  int cur = 0;
  (void)hipGetDevice(&cur);
  if (g_lba_stream && g_lba_stream_dev != cur) g_lba_stream = nullptr;  // the thread moved to another GPU
  g_lba_stream_dev = cur;
  if (!g_lba_stream) {
    // VIEO_LBA_PRIORITY = -1 / 0 / 1: lowest / default / highest stream priority for the bundle-adjustment stream.
    // Lowest by default: local mapping is the background thread of the reference and tracking must not wait for
    // it.  Next to a batched front end on another stream the bench step measured (30 steps, 205 windows per step):
    // highest 48.9 k frames/s with k_fast at 9.3 ms per launch and 0.17 ms per window; default 50.1 k / 7.6 / 0.79;
    // lowest 53.0 k / 7.7 (what k_fast takes alone) / 0.73 -- the windows' kernels are short and many and fill what the
    // front end leaves free instead of taking CUs from it.
    // One window beside a tracker is the other case: the sequential replay measured 1.03 ms per frame with the stream at
    // the DEFAULT priority against 1.08 at the lowest and 1.07 at the highest (the solve finishes sooner and the tracker
    // waits less for its write-back): the LocalMapping thread of such a host asks for it with vieo_lba_set_stream_priority(0).
    int lo = 0, hi = 0;
    const char* e = getenv("VIEO_LBA_PRIORITY");
    const int want = g_lba_priority != -2 ? g_lba_priority : (e ? atoi(e) : -1);
    if (want == 0 || hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess || lo == hi)
      VIEO_HIP_CHECK(hipStreamCreateWithFlags(&g_lba_stream, hipStreamNonBlocking));
    else
      VIEO_HIP_CHECK(hipStreamCreateWithPriority(&g_lba_stream, hipStreamNonBlocking, want < 0 ? lo : hi));
  }
  *st = g_lba_stream;
  return VIEO_OK;
}

// The windows of a call: counts, outputs preset to the inputs, which of them take part (stopped: the stop flag was up
// at entry), the solver class of those and the symbolic plan of the tile-sparse solve (built once: the full BA never
// reclassifies its edges).  Returns how many take part.
static int lba_open_windows(const LbaCall& c, bool stopped, std::vector<WinHost>& win) {
  const bool vio = c.vio();
  const int pd = c.pd(), sco = c.sco();
  const LmMode mode = c.lm_mode();
  int n_live = 0;
  for (int w = 0; w < c.W; w++) {
    WinHost& H = win[w];
    if (vio)
      H.VP = c.vparams[w], H.P = &c.vparams[w]->base, H.n_imu = c.n_imu[w];
    else {
      H.P = c.params[w];
      if (c.encs && c.encs[w]) H.ENC = c.encs[w], H.n_imu = c.encs[w]->n_edges;
    }
    H.n_kf = c.n_kf[w], H.n_mp = c.n_mp[w], H.n_obs = c.n_obs[w];  // (a rank of a sharded run may own no point of a window)
    const vieo_lba_keyframe* kfs = c.h_kfs[w];
    for (int k = 0; k < H.n_kf; k++) H.nf += !kfs[k].fixed;
    memset(&c.h_results[w], 0, sizeof(vieo_lba_result));
    lm_start(H.lm, mode, c.gba ? c.gba->iterations : H.P->its0, H.P->its1, vio ? H.VP->lambda_init : 0.0, &c.h_results[w]);
    for (int k = 0; k < H.n_kf; k++) c.h_navs_out[w][k] = kfs[k].nav;
    if (H.n_mp > 0) memcpy(c.h_points_out[w], c.h_points[w], (size_t)H.n_mp * 12);
    if (H.n_obs > 0) memset(c.h_erase[w], 0, H.n_obs);
    if (!H.nf && !sco)  // (bdimPoses = true with the scale vertex: Optimizer.cc:850)
      H.skip = true, lm_skip(H.lm, VIEO_LBA_NO_FREE_POSE);  // Optimizer.cc:1993
    else if (stopped)
      H.skip = true, lm_skip(H.lm, VIEO_LBA_ABORTED);
    if (H.skip) continue;
    n_live++;
    H.cls = solver_class(pd * H.nf + sco, c.gba && !c.sh);
    if (H.cls != 3) continue;
    std::vector<int> fx(H.n_kf), okf(H.n_obs), omp(H.n_obs), pi(H.n_imu), pj(H.n_imu);
    for (int k = 0; k < H.n_kf; k++) fx[k] = kfs[k].fixed;
    for (int i = 0; i < H.n_obs; i++) okf[i] = c.h_obs[w][i].kf, omp[i] = c.h_obs[w][i].mp;
    for (int t = 0; t < H.n_imu; t++) {
      pi[t] = vio ? c.h_imu[w][t].kf_i : H.ENC->edges[t].kf_i;
      pj[t] = vio ? c.h_imu[w][t].kf_j : H.ENC->edges[t].kf_j;
    }
    gba_sparse_plan(H.plan, H.n_kf, fx.data(), H.n_obs, okf.data(), omp.data(), H.n_mp, H.n_imu, pi.data(), pj.data(), pd, sco);
  }
  return n_live;
}

// ---- the device arena: [inputs | results (kf, X, erase, scale) | zero-initialised | scratch], the windows interleaved
// inside every region, every buffer rounded to 256 bytes.  plan_window names each buffer once -- region, the LbaDev
// pointer it feeds (whose type is its element type) and its element count; arena_layout gives them their offsets and
// arena_bind turns the offsets into pointers once a base is known (the pinned staging copy, then the device arena).
enum { R_IN, R_RES, R_ZERO, R_SCR, R_N };
struct ArenaItem {
  size_t bytes;
  bool absent;   // the window has no such buffer: the pointer is the arena's base, never dereferenced
  void* field;   // the pointer it feeds
  size_t* keep;  // where the host keeps the offset (WinHost: the results it reads back), or null
  size_t off;
};
struct WinArena {
  std::vector<ArenaItem> region[R_N];
  const int* plan = nullptr;  // the tile-sparse solve's lists (solver 3), one block in plan_lists() order
  template <class T>
  void add(int r, T*& field, size_t count, size_t* keep = nullptr) {
    region[r].push_back({count * sizeof(T), false, (void*)&field, keep, 0});
  }
  template <class T>
  void none(int r, T*& field) {
    region[r].push_back({0, true, (void*)&field, nullptr, 0});
  }
};
struct LbaLayout {
  std::vector<WinArena> win;
  size_t arena = 0, res_begin = 0, res_end = 0, zero_end = 0;  // total bytes; where the regions meet
};

// the plan's lists as the device reads them: (vector, where its pointer goes in LbaDev)
static std::vector<std::pair<const std::vector<int>*, const int**>> plan_lists(const GbaSparsePlan& P, LbaDev* D) {
  return {{&P.sch_ptr, &D->sch_ptr}, {&P.sch_i, &D->sch_i}, {&P.sch_j, &D->sch_j}, {&P.sch_diag, &D->sch_diag},
          {&P.sch_off, &D->sch_off}, {&P.col_ptr, &D->col_ptr}, {&P.tile_i, &D->tile_i}, {&P.tile_j, &D->tile_j},
          {&P.row_ptr, &D->row_ptr}, {&P.row_j, &D->row_j}, {&P.row_tile, &D->row_tile}, {&P.upd_ptr, &D->upd_ptr},
          {&P.upd, &D->upd}};
}

static void arena_layout(LbaLayout& L) {
  size_t* const ends[R_N] = {&L.res_begin, &L.res_end, &L.zero_end, &L.arena};
  for (int r = 0; r < R_N; r++) {
    for (WinArena& A : L.win)
      for (ArenaItem& it : A.region[r]) {
        if (it.absent) continue;
        it.off = L.arena;
        L.arena += (it.bytes + 255) / 256 * 256;
        if (it.keep) *it.keep = it.off;
      }
    *ends[r] = L.arena;
  }
}

// the pointers of regions [r0, r1) of a window against `base`
static void arena_bind(WinArena& A, const WinHost& H, LbaDev& D, int r0, int r1, uint8_t* base) {
  for (int r = r0; r < r1; r++)
    for (const ArenaItem& it : A.region[r]) {
      uint8_t* p = base + it.off;
      memcpy(it.field, &p, sizeof(p));
    }
  if (r0 == R_IN && H.cls == 3) {
    const int* d = A.plan;
    for (auto& l : plan_lists(H.plan, &D)) *l.second = d, d += l.first->size();
  }
}

// Schur GEMM decomposition: 64x64 block-tiles (upper) x K splits.  The number of splits is a function of the window
// alone (about 8 chunks of 16 landmarks per workgroup, cps_target), so that the summation order -- and with it the
// window's result -- does not depend on what the window is batched with; a mixed batch (ordinary windows of one
// tile next to bLarge ones of six) launches the largest tile x split count and the others' workgroups exit.
// Measured per call of 205 windows, cps_target = 3 / 6 / 12 / 24: Schur 4.9 / 4.6 / 4.7 / 6.1 ms, k_lba_assemble
// (which sums the partials) 2.1 / 1.6 / 1.2 / 1.1 ms.  The full BA keeps few splits: its tiles are many and
// mostly skipped (k_lba_occ).
static int schur_tiles(int npm) {  // npm: rows of the visual system
  const int RB = (npm + 63) / 64, CB = (npm + 64) / 64;
  return RB * CB - RB * (RB - 1) / 2;
}
static int schur_ksplit(int npm, int nmp, bool gba) {
  const int cps_target = 8;
  const int nch = (nmp + kChunkLm - 1) / kChunkLm, nbt = std::max(1, schur_tiles(npm));
  if (gba) return std::max(1, std::min(std::min(nch, 16), 768 / nbt));
  return std::max(1, std::min(std::min((nch + cps_target - 1) / cps_target, 32), std::max(1, 512 / nbt)));
}

// The launch grids and class tables of a batch, computed once: every kernel covers all windows of the batch, so each
// grid is the largest any window needs.
struct LbaGrids {
  int ge = 1, gm = 1, gq = 1, gr = 1;  // blocks of 256 edges / 256 points / 64 points / max(256 points, 256 key frames)
  int schur = 0, schur_off = 0;        // Schur GEMM: diagonal / off-diagonal tiles x splits of the dense windows
  int schur_t = 0, schur_t_off = 0;    //   the same over the planned tiles of the tile-sparse windows
  int cls_max[4] = {0, 0, 0, 0};       // per solver class: the largest system of the class (0: the class is empty)
  int cls_first[5] = {0, 0, 0, 0, 0};  // cls_order[cls_first[c] .. cls_first[c + 1]): the windows of class c
  std::vector<int> cls_order;          // (alive until the call returns: its copy to the device is asynchronous)
  int nb16 = 0, nbg = 0;               // 16 x 16 blocks of the largest class-0 / class-1 system
  // the tile-sparse solve: tile rows, the assembly's elements; per panel k the rows under the diagonal tile and the
  // update targets
  int sp_nt = 0;
  size_t sp_elems = 0;
  std::vector<int> sp_panel_grid, sp_syrk_grid;
  int occ_max = 0, max_chunks = 1, max_imu = 0, max_nf = 0, max_mp = 0;
  bool any_multicam = false;
  // k_lba_tail (one launch for the tail of a trial) for calls of a few windows: one window beside the tracker 5.0 -> 4.9 ms,
  // W = 4 equal, but W = 16 / 64 windows 2.80 -> 3.02 / 5.07 -> 6.47 ms per call -- its residual pass runs four lanes per
  // point over the point's edges (that is what makes it independent of the other workgroups), which is latency-bound and
  // loses to k_lba_error's lane per edge once the launch ramps are amortised over many windows.  Batches take the
  // four-launch form (the tail without the fold + k_lba_reduce over its partials measured 3.9 against 2.9 ms of kernel
  // time per 205-window step).  Both halves of k_lba_build in one launch: calls of a few windows as well.
  bool fused_tail = false, fused_build = false;
  size_t shard_sys = 0;  // sharded run: doubles of the windows' packed reduced systems in the reduction buffer
};

// A window's descriptor (everything but the arena pointers) and its rows of the arena table.
static void plan_window(const LbaCall& c, WinHost& H, LbaDev& D, WinArena& A, LbaGrids& G) {
  const bool vio = c.vio(), gba = c.gba != nullptr, tiles = H.cls == 3;
  const int sco = c.sco(), pd = c.pd(), nf = H.nf;
  const int npm = 6 * nf + sco;   // rows of the visual system: PR blocks (+ the scale vertex)
  const int npf = pd * nf + sco;  // full reduced system
  const int sp_rows = (npm + 63) / 64 * 64, ldS = (npm + 64) / 64 * 64;
  const int ksplit = schur_ksplit(npm, H.n_mp, gba);  // (the tile-sparse solve keeps the dense split: the same sums)
  const GbaSparsePlan& PL = H.plan;
  const size_t n_obs = H.n_obs, n_mp = H.n_mp, n_kf = H.n_kf, n_edge = std::max(H.n_imu, 1);
  const size_t blk256 = (n_obs + 255) / 256, blk64 = (n_mp + 63) / 64;
  // chunks of the key frames' edge lists: sum over the free key frames of ceil(edges / kBuildChunk) <= this bound
  const size_t nchk = n_obs / kBuildChunk + nf + 1;
  memset(&D, 0, sizeof(D));
  A.region[R_IN].reserve(11), A.region[R_RES].reserve(4), A.region[R_ZERO].reserve(2), A.region[R_SCR].reserve(40);
  D.nb = (npf + 1 + kNB - 1) / kNB * kNB;  // + the right-hand-side row
  if (H.cls == 1) D.nb = (npf + 16) >> 4;  // 16 x 16 blocks of the bordered matrix

  A.add(R_IN, D.obs, n_obs);
  A.add(R_IN, D.mp_first, n_mp), A.add(R_IN, D.mp_count, n_mp);
  A.add(R_IN, D.kf_edge_first, n_kf + 1), A.add(R_IN, D.kf_edge_idx, n_obs);
  A.add(R_IN, D.ocam, n_obs);
  if (vio || H.ENC) {
    A.add(R_IN, D.imu, n_edge);
    A.add(R_IN, D.kf_in, n_kf), A.add(R_IN, D.kf_out, n_kf), A.add(R_IN, D.close, n_mp);
  }
  if (tiles) A.add(R_IN, A.plan, PL.list_ints());

  A.add(R_RES, D.kf, n_kf, &H.o_kf), A.add(R_RES, D.X, 3 * n_mp, &H.o_X), A.add(R_RES, D.erase, n_obs, &H.o_erase);
  A.add(R_RES, D.scl, 2, &H.o_scl);

  A.add(R_ZERO, D.level, n_obs), A.add(R_ZERO, D.err, 3 * n_obs);

  A.add(R_SCR, D.kf_bak, n_kf), A.add(R_SCR, D.X_bak, 3 * n_mp);
  A.add(R_SCR, D.xf, n_kf * (size_t)std::max(1, H.P->n_cams));
  A.add(R_SCR, D.mp_act, n_mp);
  A.add(R_SCR, D.CB, (n_obs + 1) * 18);  // + the zero block
  if (sco)
    A.add(R_SCR, D.Bs, 3 * std::max<size_t>(n_mp, 1));
  else
    A.none(R_SCR, D.Bs);
  A.add(R_SCR, D.Sp, tiles ? PL.schur_bytes(ksplit) / 8 : (size_t)ksplit * sp_rows * ldS);
  A.add(R_SCR, D.Hll, 9 * n_mp), A.add(R_SCR, D.bl, 3 * n_mp);
  A.add(R_SCR, D.Hpp, (size_t)std::max(nf, 1) * 36);
  if (tiles) {  // no dense Hs; the tile pool, W of a panel for every row
    A.none(R_SCR, D.Hs);
    A.add(R_SCR, D.Hb, PL.pool_bytes() / 8), A.add(R_SCR, D.Wp, PL.panel_bytes() / 8), A.add(R_SCR, D.big_fail, 64);
  } else {
    if (H.cls == 0)  // formed in the solve's LDS
      A.none(R_SCR, D.Hs);
    else
      A.add(R_SCR, D.Hs, (size_t)npf * npf);
    if (H.cls == 2)
      A.add(R_SCR, D.Hb, (size_t)D.nb * D.nb), A.add(R_SCR, D.Wp, (size_t)D.nb * kNB), A.add(R_SCR, D.big_fail, 64);
    else if (H.cls == 1)
      A.add(R_SCR, D.Hb, ldg_scratch_doubles(D.nb)), A.none(R_SCR, D.Wp), A.none(R_SCR, D.big_fail);
    else
      A.none(R_SCR, D.Hb), A.none(R_SCR, D.Wp), A.none(R_SCR, D.big_fail);
  }
  A.add(R_SCR, D.bp, npm), A.add(R_SCR, D.bs, npf), A.add(R_SCR, D.xp, npf);
  A.add(R_SCR, D.bfull, npf);
  A.add(R_SCR, D.Ae, n_edge * 930);
  A.add(R_SCR, D.gchi0, n_edge), A.add(R_SCR, D.gchi, n_edge);
  A.add(R_SCR, D.part0, blk256), A.add(R_SCR, D.part, blk256);
  A.add(R_SCR, D.part_m, blk64), A.add(R_SCR, D.pmax, blk64);
  A.add(R_SCR, D.part_t, std::max<size_t>(blk64, 1)), A.add(R_SCR, D.tail_cnt, 64);
  A.add(R_SCR, D.chunk_first, nf + 1), A.add(R_SCR, D.chunk_cnt, nf + 1);
  A.add(R_SCR, D.chunk_kf, nchk), A.add(R_SCR, D.chunk_part, nchk * 33);
  A.add(R_SCR, D.kf_list, n_kf), A.add(R_SCR, D.tab, (size_t)std::max(nf, 1) * n_mp);
  A.add(R_SCR, D.sc_sys, 6 * nf + 2), A.add(R_SCR, D.psc, blk64 * 2);
  A.add(R_SCR, D.kf_act, n_kf);
  A.add(R_SCR, D.occ, (size_t)((npm + 64) / 64) * ((n_mp + kChunkLm - 1) / kChunkLm));

  D.n_obs = H.n_obs, D.n_mp = H.n_mp, D.n_kf = H.n_kf, D.nf_cap = nf;
  D.ldS = ldS, D.sp_stride = tiles ? PL.n_sch_tiles() * kGbaTileElems : (size_t)sp_rows * ldS, D.ksplit = ksplit;
  D.cam.fx = H.P->fx, D.cam.fy = H.P->fy, D.cam.cx = H.P->cx, D.cam.cy = H.P->cy, D.cam.bf = H.P->bf;
  memcpy(D.cam.Rcb, H.P->Rcb, 72);
  memcpy(D.cam.tcb, H.P->tcb, 24);
  D.n_cams = H.P->n_cams;
  for (int ci = 0; ci < H.P->n_cams; ci++) {
    const vieo_camera& cam = H.P->cams[ci];
    CamD& d = D.cams[ci];
    d.fx = cam.fx, d.fy = cam.fy, d.cx = cam.cx, d.cy = cam.cy, d.bf = 0;
    memcpy(d.Rcb, cam.Rcb, 72), memcpy(d.tcb, cam.tcb, 24);
    d.model = cam.model, d.num_k = cam.model == VIEO_CAM_RADTAN ? cam.num_k : 0;
    for (int q = 0; q < 8; q++) d.k[q] = (double)cam.dist[q];
  }
  // thHuberMono = sqrt(5.991) in the local BAs, thHuber2D = sqrt(5.99) in the global ones (Optimizer.cc:1063,1445)
  D.dMono = (double)(float)sqrt(gba ? 5.99 : 5.991), D.dStereo = (double)(float)sqrt(7.815);
  D.pd = pd, D.n_imu = H.n_imu;
  D.scale_opt = sco;
  D.use_occ = gba ? 1 : 0;
  D.solver = H.cls;
  D.fold_kernel = c.W <= 4 ? 0 : 1;
  if (tiles) {
    D.n_sch_diag = (int)PL.sch_diag.size(), D.n_sch_off = (int)PL.sch_off.size();
    D.nt = PL.nt, D.n_tiles = (int)PL.n_tiles();
  }
  if (vio) {  // const float chi2Mono = 5.991; 1.5 * chi2Mono; literal 7.815 (Optimizer.cc:347,603-620)
    D.thMono = (double)5.991f, D.thMonoClose = 1.5 * (double)5.991f, D.thStereo = 7.815;
    memcpy(D.gw, H.VP->gw, 24);
    memcpy(D.qRbe, H.VP->qRbe, 32), memcpy(D.pbe, H.VP->pbe, 24);
    D.th_dist_far = (!gba && H.VP->th_dist_far > 0 && std::isfinite(H.VP->th_dist_far)) ? (double)H.VP->th_dist_far : 0.0;
  } else {
    D.thMono = D.thMonoClose = 5.991, D.thStereo = 7.815;
    if (H.ENC) memcpy(D.qRbe, H.ENC->qRbe, 32), memcpy(D.pbe, H.ENC->pbe, 24);
  }

  // the window's share of the batch's grids
  if (tiles) {
    G.schur_t = std::max(G.schur_t, (int)PL.sch_diag.size() * ksplit);
    G.schur_t_off = std::max(G.schur_t_off, (int)PL.sch_off.size() * ksplit);
    G.sp_nt = std::max(G.sp_nt, PL.nt), G.sp_elems = std::max(G.sp_elems, PL.n_tiles() * kGbaTileElems);
    G.sp_panel_grid.resize(G.sp_nt, 1), G.sp_syrk_grid.resize(G.sp_nt, 0);
    for (int k = 0; k < PL.nt; k++) {
      G.sp_panel_grid[k] = std::max(G.sp_panel_grid[k], 1 + ((PL.col_ptr[k + 1] - PL.col_ptr[k] - 1) * kNB + 255) / 256);
      G.sp_syrk_grid[k] = std::max(G.sp_syrk_grid[k], PL.upd_ptr[k + 1] - PL.upd_ptr[k]);
    }
  } else {
    const int RBw = (npm + 63) / 64;
    G.schur = std::max(G.schur, RBw * ksplit);
    G.schur_off = std::max(G.schur_off, (schur_tiles(npm) - RBw) * ksplit);
  }
  // (at least one workgroup each: an empty landmark shard still launches everything)
  G.ge = std::max(G.ge, (H.n_obs + 255) / 256), G.gm = std::max(G.gm, (H.n_mp + 255) / 256);
  G.gq = std::max(G.gq, (H.n_mp + 63) / 64), G.gr = std::max(std::max(G.gr, G.gm), (H.n_kf + 255) / 256);
  G.max_chunks = std::max(G.max_chunks, (int)nchk), G.max_imu = std::max(G.max_imu, H.n_imu);
  G.max_nf = std::max(G.max_nf, nf), G.max_mp = std::max(G.max_mp, H.n_mp);
  G.any_multicam |= H.P->n_cams > 0;
  G.cls_max[H.cls] = std::max(G.cls_max[H.cls], npf);
}

// Descriptors, arena table and grids of the windows that take part; the offsets of everything.
static void lba_layout(const LbaCall& c, std::vector<WinHost>& win, std::vector<LbaDev>& devs, LbaLayout& L, LbaGrids& G) {
  const int W = c.W;
  L.win.resize(W);
  for (int w = 0; w < W; w++)
    if (!win[w].skip) plan_window(c, win[w], devs[w], L.win[w], G);
  arena_layout(L);
  G.occ_max = ((6 * G.max_nf + c.sco() + 64) / 64) * ((G.max_mp + kChunkLm - 1) / kChunkLm);
  for (int cl = 0; cl < 4; cl++) {
    G.cls_first[cl] = (int)G.cls_order.size();
    for (int w = 0; w < W; w++)
      if (!win[w].skip && win[w].cls == cl) G.cls_order.push_back(w);
  }
  G.cls_first[4] = (int)G.cls_order.size();
  G.nb16 = (G.cls_max[0] + 16) >> 4, G.nbg = (G.cls_max[1] + 16) >> 4;
  G.fused_tail = G.fused_build = W <= 4;
}

template <class T>
static T* staged(const T* p) {  // a descriptor bound to the staging copy: the host fills what the device will only read
  return const_cast<T*>(p);
}

// the encoder half of a key-frame pair's edge (EdgeEncNavStatePR): measurement and information, x 1e-2 when kf_i is fixed
// (Optimizer.cc:323-347, 2030-2033); d.measE / d.InfoE are zero on entry
static bool fill_enc_edge(LbaImu& d, const vieo_enc_preint& enc, bool fixed_i, int robust) {
  d.has_enc = enc.dt != 0, d.enc_robust = robust;
  if (!d.has_enc) return true;
  memcpy(d.measE, enc.delx, 48);
  if (!inverse_n(enc.Sigma, d.InfoE, 6)) return false;
  if (fixed_i)
    for (int q = 0; q < 36; q++) d.InfoE[q] *= 1e-2;
  return true;
}

// kf_in / kf_out: the pair edge ending / starting at every key frame, -1 = none
static void fill_chain(const LbaDev& S, const WinHost& H) {
  const LbaImu* im = S.imu;
  int *kin = staged(S.kf_in), *kout = staged(S.kf_out);
  for (int k = 0; k < H.n_kf; k++) kin[k] = kout[k] = -1;
  for (int t = 0; t < H.n_imu; t++) kout[im[t].i] = t, kin[im[t].j] = t;
}

// The inputs of window w into the pinned copy of the arena (index structures, key frames, inertial / encoder edges with
// their information matrices, points).  S: the window's descriptor with its input and result pointers bound to that copy.
static int fill_window(const LbaCall& c, int w, const WinHost& H, const LbaDev& S) {
  const vieo_lba_obs* ob = c.h_obs[w];
  const vieo_lba_keyframe* kfs = c.h_kfs[w];
  const int enc_robust = c.gba ? c.gba->robust != 0 : 1;
  {  // the device sees plain key-frame indices; the camera index travels in its own byte array
    vieo_lba_obs* so = staged(S.obs);
    uint8_t* ocam = staged(S.ocam);
    for (int i = 0; i < H.n_obs; i++) {
      if (!lba_obs_ok(ob, i, H.n_mp, H.n_kf, H.P->n_cams)) return lba_obs_invalid();
      so[i] = ob[i];
      so[i].kf = ob[i].kf & 0xFFFFFF;
      ocam[i] = (uint8_t)((ob[i].kf >> 24) & 15);
    }
    ob = so;
  }
  int *mp_first = staged(S.mp_first), *mp_count = staged(S.mp_count);
  int *kf_first = staged(S.kf_edge_first), *kf_idx = staged(S.kf_edge_idx);
  memset(mp_first, 0, (size_t)H.n_mp * 4), memset(mp_count, 0, (size_t)H.n_mp * 4);
  memset(kf_first, 0, (size_t)(H.n_kf + 1) * 4);
  for (int i = 0; i < H.n_obs; i++) {
    const int m = ob[i].mp;
    if (mp_count[m] == 0) mp_first[m] = i;
    mp_count[m]++;
    kf_first[ob[i].kf + 1]++;
  }
  for (int k = 0; k < H.n_kf; k++) kf_first[k + 1] += kf_first[k];
  std::vector<int> fill(kf_first, kf_first + H.n_kf);
  for (int i = 0; i < H.n_obs; i++) kf_idx[fill[ob[i].kf]++] = i;
  LbaKf* kf = S.kf;
  for (int k = 0; k < H.n_kf; k++) {
    memcpy(kf[k].p, kfs[k].nav.p, 24);
    kf[k].qw = kfs[k].nav.q[0], kf[k].qx = kfs[k].nav.q[1];
    kf[k].qy = kfs[k].nav.q[2], kf[k].qz = kfs[k].nav.q[3];
    kf[k].col = -1, kf[k].fixed = kfs[k].fixed ? 1 : 0;
    memcpy(kf[k].v, kfs[k].nav.v, 24), memcpy(kf[k].dbg, kfs[k].nav.dbg, 24), memcpy(kf[k].dba, kfs[k].nav.dba, 24);
    memcpy(kf[k].bg, kfs[k].nav.bg, 24), memcpy(kf[k].ba, kfs[k].nav.ba, 24);
  }
  if (H.VP) {  // inertial edges (Optimizer.cc:226-311)
    LbaImu* im = staged(S.imu);
    for (int t = 0; t < H.n_imu; t++) {
      const vieo_lba_imu_edge& e = c.h_imu[w][t];
      LbaImu& d = im[t];
      d.i = e.kf_i, d.j = e.kf_j, d.M = e.imu;
      const bool bfixedkf = kfs[e.kf_i].fixed != 0;
      d.has_imu = e.imu.dt != 0, d.robust = c.gba ? c.gba->robust != 0 : (bfixedkf || H.VP->rec_init);
      memset(d.InfoI, 0, sizeof(d.InfoI));
      if (d.has_imu) {
        if (!inverse_n(e.imu.Sigma, d.InfoI, 9)) {
          set_error("visual-inertial local BA: singular pre-integration covariance");
          return VIEO_E_INVALID;
        }
        if (bfixedkf)
          for (int q = 0; q < 81; q++) d.InfoI[q] *= 1e-2;
      }
      double deltatij = e.imu.dt ? e.imu.dt : e.dt_kf;
      const float EPS_MIN_DT = 1e-6f;
      if (deltatij <= EPS_MIN_DT) deltatij = 15;  // Optimizer.cc:271-275
      d.infoBg = H.VP->inv_sigma_bg2 / deltatij * (bfixedkf ? 1e-2 : 1.0);
      d.infoBa = H.VP->inv_sigma_ba2 / deltatij * (bfixedkf ? 1e-2 : 1.0);
      memset(d.InfoE, 0, sizeof(d.InfoE)), memset(d.measE, 0, sizeof(d.measE));
      if (!fill_enc_edge(d, e.enc, bfixedkf, enc_robust)) {
        set_error("visual-inertial local BA: singular encoder covariance");
        return VIEO_E_INVALID;
      }
    }
    fill_chain(S, H);
    if (c.h_close[w])
      memcpy(staged(S.close), c.h_close[w], H.n_mp);
    else
      memset(staged(S.close), 0, H.n_mp);
  } else if (H.ENC) {  // encoder edges only: no inertial residual, no bias random walk
    LbaImu* im = staged(S.imu);
    for (int t = 0; t < H.n_imu; t++) {
      const vieo_lba_enc_edge& e = H.ENC->edges[t];
      LbaImu& d = im[t];
      memset(&d, 0, sizeof(d));
      d.i = e.kf_i, d.j = e.kf_j;
      if (!fill_enc_edge(d, e.enc, kfs[e.kf_i].fixed != 0, enc_robust)) {
        set_error("local BA: singular encoder covariance");
        return VIEO_E_INVALID;
      }
    }
    fill_chain(S, H);
    memset(staged(S.close), 0, H.n_mp);
  }
  for (int i = 0; i < H.n_mp * 3; i++) S.X[i] = (double)c.h_points[w][i];
  memset(S.erase, 0, H.n_obs);
  S.scl[0] = S.scl[1] = 1.0;  // pvScale->setEstimate(1.) (Optimizer.cc:845)
  if (H.cls == 3) {
    int* d = staged(S.sch_ptr);  // the first of plan_lists(): the block's start
    LbaDev unused;
    for (auto& l : plan_lists(H.plan, &unused))
      if (!l.first->empty()) memcpy(d, l.first->data(), l.first->size() * 4), d += l.first->size();
  }
  return VIEO_OK;
}

// Staging: the inputs of every window into the pinned copy `hs` of the arena.  Windows are independent and the work is
// memory copies, so a large batch is split over a few host threads (6.6 ms on one thread for the 103 windows of a
// bench step).
static int lba_stage(const LbaCall& c, const std::vector<WinHost>& win, std::vector<LbaDev>& devs, LbaLayout& L, uint8_t* hs) {
  std::vector<int> live;
  for (int w = 0; w < c.W; w++)
    if (!win[w].skip) live.push_back(w), arena_bind(L.win[w], win[w], devs[w], R_IN, R_ZERO, hs);
  auto fill = [&](int w) { return fill_window(c, w, win[w], devs[w]); };
  const int hw = (int)std::thread::hardware_concurrency();
  const int nt = std::max(1, std::min(std::min(8, hw > 0 ? hw : 1), (int)live.size() / 8));
  std::vector<int> rcs(live.size(), VIEO_OK);
  if (nt <= 1) {
    for (size_t i = 0; i < live.size(); i++)
      if ((rcs[i] = fill(live[i])) != VIEO_OK) return rcs[i];
    return VIEO_OK;
  }
  std::vector<std::thread> th;
  for (int t = 0; t < nt; t++)
    th.emplace_back([&, t] {
      for (size_t i = t; i < live.size(); i += nt) rcs[i] = fill(live[i]);
    });
  for (auto& x : th) x.join();
  for (size_t i = 0; i < live.size(); i++)
    if (rcs[i] != VIEO_OK) return fill(live[i]);  // again on this thread: the error text is thread-local
  return VIEO_OK;
}

// The device side of the descriptors: the arena (reserved here), the pointers into it, a sharded run's slices of the
// reduction buffer.
static int lba_describe(const LbaCall& c, const std::vector<WinHost>& win, std::vector<LbaDev>& devs, LbaLayout& L, LbaGrids& G) {
  const int W = c.W;
  int rc;
  if (G.cls_max[3] > 0) {
    // the tile-sparse solve's limit is device memory: its pool, Schur tiles and lists are part of the arena
    size_t fr = 0, tot = 0;
    int cur = 0;
    (void)hipGetDevice(&cur);
    VIEO_HIP_CHECK(hipMemGetInfo(&fr, &tot));
    const size_t have = fr + (g_arena.p && g_arena.dev == cur ? g_arena.cap : 0);
    if (L.arena > have) {
      size_t plan_b = 0;
      for (int w = 0; w < W; w++)
        if (win[w].cls == 3) plan_b += win[w].plan.bytes(devs[w].ksplit);
      set_error("bundle adjustment: the tile-sparse solve needs %zu bytes of device memory (%zu of them the tile pool, "
                "Schur tiles and plan), %zu are free",
                L.arena, plan_b, have);
      return VIEO_E_CAPACITY;
    }
  }
  if ((rc = g_arena.ensure(L.arena)) != VIEO_OK) return rc;
  for (int w = 0; w < W; w++)
    if (win[w].cls == 3) {
      const GbaSparsePlan& P = win[w].plan;
      std::lock_guard<std::mutex> g(g_lba_kt_mutex);
      g_lba_sparse_stats[0] = (long long)P.n_tiles(), g_lba_sparse_stats[1] = (long long)P.nt * (P.nt + 1) / 2;
      g_lba_sparse_stats[2] = (long long)P.n_sch_tiles(), g_lba_sparse_stats[3] = (long long)P.vrb * P.vcb - (long long)P.vrb * (P.vrb - 1) / 2;
      g_lba_sparse_stats[4] = (long long)P.bytes(devs[w].ksplit), g_lba_sparse_stats[5] = (long long)L.arena;
    }
  if ((rc = g_small.ensure((size_t)W * (sizeof(LbaDev) + sizeof(WinCtl) + sizeof(WinOut) + sizeof(int)))) != VIEO_OK) return rc;
  if ((rc = g_small_h.ensure((size_t)W * (sizeof(WinCtl) + sizeof(WinOut) + 32))) != VIEO_OK) return rc;
  for (int w = 0; w < W; w++)
    if (!win[w].skip) arena_bind(L.win[w], win[w], devs[w], R_IN, R_N, g_arena.as<uint8_t>());
  if (const LbaShard* sh = c.sh) {
    for (int w = 0; w < W; w++) {
      if (win[w].skip) continue;
      devs[w].red = sh->d_buf + G.shard_sys;
      G.shard_sys += shard_sys_doubles(devs[w].nf_cap, c.sco());
    }
    if (G.shard_sys + 4 * (size_t)W > sh->cap) {
      set_error("sharded local BA: reduction buffer too small (%zu doubles needed)", G.shard_sys + 4 * (size_t)W);
      return VIEO_E_CAPACITY;
    }
    for (int w = 0; w < W; w++) devs[w].red_sc = sh->d_buf + G.shard_sys + 4 * (size_t)w;
  }
  return VIEO_OK;
}

struct LbaBufs {  // the small per-window records of a call, on the device and pinned on the host
  LbaDev* dD;
  WinCtl* dC;
  WinOut* dO;
  int* dWins;  // the windows grouped by solver class: [class 0 | class 1 | class 2 | class 3] (LbaGrids::cls_order)
  WinCtl* ctl;
  WinOut* out;
  double* h_sc;  // reduced scalars of a sharded run
};

static LbaBufs lba_bufs(int W) {
  LbaBufs B;
  B.dD = g_small.as<LbaDev>();
  B.dC = (WinCtl*)(B.dD + W), B.dO = (WinOut*)(B.dC + W), B.dWins = (int*)(B.dO + W);
  B.ctl = (WinCtl*)g_small_h.p, B.out = (WinOut*)(B.ctl + W), B.h_sc = (double*)(B.out + W);
  return B;
}

// Everything a call sends ahead of its rounds: the staged arena, the descriptors, the class table.
static int lba_enqueue(const LbaCall& c, const LbaLayout& L, const std::vector<LbaDev>& devs, const LbaGrids& G,
                       const LbaBufs& B, const uint8_t* hs, hipStream_t st) {
  const int W = c.W;
  uint8_t* base = g_arena.as<uint8_t>();
  VIEO_HIP_CHECK(hipMemcpyAsync(base, hs, L.res_end, hipMemcpyHostToDevice, st));
  VIEO_HIP_CHECK(hipMemsetAsync(base + L.res_end, 0, L.zero_end - L.res_end, st));
  VIEO_HIP_CHECK(hipMemcpyAsync(B.dD, devs.data(), (size_t)W * sizeof(LbaDev), hipMemcpyHostToDevice, st));
  VIEO_HIP_CHECK(hipMemsetAsync(B.dO, 0, (size_t)W * sizeof(WinOut), st));
  if (!G.cls_order.empty())
    VIEO_HIP_CHECK(hipMemcpyAsync(B.dWins, G.cls_order.data(), G.cls_order.size() * sizeof(int), hipMemcpyHostToDevice, st));
  if (G.cls_max[1] > 0)
    VIEO_HIP_CHECK(hipFuncSetAttribute((const void*)k_lba_ldltg<kLdGThreads>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)ldg_lds_bytes(G.nbg)));
  if (G.cls_max[0] > 0)
    VIEO_HIP_CHECK(hipFuncSetAttribute((const void*)k_lba_ldlt16<kLd16Threads>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)ld16_lds_bytes(G.nb16)));
  return VIEO_OK;
}

// The tiled LDL^T over many workgroups, dense (class 2) or over the stored tiles of the fill pattern (class 3): nt
// panels -- panel_grid(k) the rows under panel k's diagonal tile, syrk_grid(k) its update targets -- then the back
// substitution of n unknowns.
template <bool TILES, class PanelGrid, class SyrkGrid>
static void launch_big_ldlt(LbaKTimer& KT, int kc, const LbaBufs& B, int W, hipStream_t st, int nt, int n,
                            PanelGrid panel_grid, SyrkGrid syrk_grid) {
  LbaDev* dD = B.dD;
  WinCtl* dC = B.dC;
  WinOut* dO = B.dO;
  for (int k = 0; k < nt; k++) {
    KT.launch(kc, [&] { hipLaunchKernelGGL(k_big_panel<TILES>, dim3(panel_grid(k), W), dim3(256), 0, st, dD, dC, k); });
    if (syrk_grid(k) > 0)
      KT.launch(kc, [&] { hipLaunchKernelGGL(k_big_syrk<TILES>, dim3(syrk_grid(k), W), dim3(256), 0, st, dD, dC, k); });
  }
  for (int sb = 0; sb < (n + kNB - 1) / kNB; sb++)
    KT.launch(kc, [&] { hipLaunchKernelGGL(k_big_back_step<TILES>, dim3(1 + (n + 255) / 256, W), dim3(256), 0, st, dD, dC, sb); });
  KT.launch(kc, [&] { hipLaunchKernelGGL(k_big_finish<TILES>, dim3(W), dim3(256), 0, st, dD, dC, dO); });
}

// The launch schedule of one round.  any: the windows' control words or-ed together; cls_trial[c]: a window of solver
// class c takes a trial this round.
static int launch_round(const LbaCall& c, const LbaGrids& G, const LbaBufs& B, LbaKTimer& KT, int any,
                        const bool* cls_trial, hipStream_t st) {
  const LbaShard* sh = c.sh;
  const int W = c.W, sco = c.sco();
  const int ge = G.ge, gq = G.gq, gr = G.gr, max_chunks = G.max_chunks, max_imu = G.max_imu, max_nf = G.max_nf;
  const int* cls_max = G.cls_max;
  const int* cls_first = G.cls_first;
  LbaDev* dD = B.dD;
  WinCtl* dC = B.dC;
  WinOut* dO = B.dO;
  int* dWins = B.dWins;
  int rc;
  VIEO_HIP_CHECK(hipMemcpyAsync(dC, B.ctl, (size_t)W * sizeof(WinCtl), hipMemcpyHostToDevice, st));
  if (any & LBA_RESTORE) KT.launch(KC_OTHER, [&] { hipLaunchKernelGGL(k_lba_restore, dim3(gr, W), dim3(256), 0, st, dD, dC); });
  if (any & (LBA_CLASS0 | LBA_CLASS1)) KT.launch(KC_OTHER, [&] { hipLaunchKernelGGL(k_lba_classify, dim3(ge, W), dim3(256), 0, st, dD, dC); });
  if (any & LBA_PRELEVEL)
    for (int ph = 0; ph < 3; ph++) KT.launch(KC_OTHER, [&] { hipLaunchKernelGGL(k_lba_prelevel, dim3(ge, W), dim3(256), 0, st, dD, dC, ph); });
  if (any & LBA_BEGIN) {
    KT.launch(KC_BEGIN, [&] { hipLaunchKernelGGL(k_lba_zero, dim3(64, W), dim3(256), 0, st, dD, dC); });
    KT.launch(KC_BEGIN, [&] { hipLaunchKernelGGL(k_lba_begin, dim3(W), dim3(1024), 0, st, dD, dC, dO); });
    if (c.gba) KT.launch(KC_BEGIN, [&] { hipLaunchKernelGGL(k_lba_occ, dim3(std::max(1, (G.occ_max + 255) / 256), W), dim3(256), 0, st, dD, dC); });
    KT.launch(KC_ERROR, [&] { hipLaunchKernelGGL(k_lba_error, dim3(ge, W), dim3(256), 0, st, dD, dC, 0); });
  }
  if (any & LBA_BUILD) {
    auto build2 = [&](auto mc, auto sc) {  // point half, key-frame half
      constexpr bool MC = decltype(mc)::value, SC = decltype(sc)::value;
      if (G.fused_build) {  // one launch for both halves
        KT.launch(KC_BUILD, [&] { hipLaunchKernelGGL((k_lba_build<MC, SC, 2>), dim3(gq + max_chunks + max_imu, W), dim3(256), 0, st, dD, dC, max_chunks, gq); });
        if (W > 4) KT.launch(KC_BUILD, [&] { hipLaunchKernelGGL(k_lba_build_fold, dim3(std::max(1, max_nf), W), dim3(64), 0, st, dD, dC); });
        return;
      }
      KT.launch(KC_BUILD, [&] { hipLaunchKernelGGL((k_lba_build<MC, SC, 0>), dim3(gq, W), dim3(256), 0, st, dD, dC, 0, 0); });
      KT.launch(KC_BUILD, [&] { hipLaunchKernelGGL((k_lba_build<MC, SC, 1>), dim3(max_chunks, W), dim3(256), 0, st, dD, dC, max_chunks, 0); });
      if (W > 4) KT.launch(KC_BUILD, [&] { hipLaunchKernelGGL(k_lba_build_fold, dim3(std::max(1, max_nf), W), dim3(64), 0, st, dD, dC); });
    };
    if (sco) {
      if (G.any_multicam)
        build2(std::true_type(), std::true_type());
      else
        build2(std::false_type(), std::true_type());
      KT.launch(KC_BUILD, [&] { hipLaunchKernelGGL(k_lba_scale_fold, dim3(W), dim3(256), 0, st, dD, dC); });
    } else if (G.any_multicam)
      build2(std::true_type(), std::false_type());
    else
      build2(std::false_type(), std::false_type());
    if (!G.fused_build && max_imu > 0) KT.launch(KC_GENERIC, [&] { hipLaunchKernelGGL(k_lba_generic, dim3(max_imu, W), dim3(64), 0, st, dD, dC, 0); });
  }
  if (any & LBA_BEGIN) KT.launch(KC_BEGIN, [&] { hipLaunchKernelGGL(k_lba_lambda, dim3(W), dim3(256), 0, st, dD, dC, dO); });
  if (!(any & LBA_TRIAL)) return VIEO_OK;
  const bool sparse_trial = cls_max[3] > 0 && cls_trial[3];
  if (cls_max[0] > 0 || cls_max[1] > 0 || cls_max[2] > 0) {
    KT.launch(KC_SCHUR, [&] { hipLaunchKernelGGL(k_lba_schur<false>, dim3(std::max(1, G.schur), W), dim3(256), 0, st, dD, dC, dO); });
    if (G.schur_off > 0)
      KT.launch(KC_SCHUR, [&] { hipLaunchKernelGGL(k_lba_schur<true>, dim3(G.schur_off, W), dim3(256), 0, st, dD, dC, dO); });
  }
  if (sparse_trial) {  // the planned tiles only
    KT.launch(KC_SCHUR, [&] { hipLaunchKernelGGL((k_lba_schur<false, true>), dim3(std::max(1, G.schur_t), W), dim3(256), 0, st, dD, dC, dO); });
    if (G.schur_t_off > 0)
      KT.launch(KC_SCHUR, [&] { hipLaunchKernelGGL((k_lba_schur<true, true>), dim3(G.schur_t_off, W), dim3(256), 0, st, dD, dC, dO); });
  }
  if (sh) {  // the one exchange step of the path: sum the reduced visual system over the ranks
    KT.launch(KC_OTHER, [&] { hipLaunchKernelGGL(k_lba_pack, dim3((unsigned)((shard_sys_doubles(max_nf, sco) + 255) / 256), W), dim3(256), 0, st,
                       dD, dC); });
    if ((rc = shard_exchange(sh, sh->d_buf, G.shard_sys, st)) != VIEO_OK) return rc;
  }
  for (int cl = 1; cl < 3; cl++) {  // (class 0: k_lba_ldlt16 forms its system itself)
    const int nw = cls_first[cl + 1] - cls_first[cl];
    if (nw <= 0 || !cls_trial[cl]) continue;
    const unsigned gx = (unsigned)(((size_t)cls_max[cl] * cls_max[cl] + 255) / 256);
    KT.launch(KC_ASSEMBLE, [&] { hipLaunchKernelGGL(k_lba_assemble, dim3(gx, nw), dim3(256), 0, st, dD, dC, dO, dWins + cls_first[cl]); });
  }
  if (cls_max[2] > 0 && cls_trial[2]) {
    const int n = cls_max[2], nbm = (n + 1 + kNB - 1) / kNB * kNB, ntm = nbm / kNB;
    KT.launch(KC_LDLT, [&] { hipLaunchKernelGGL(k_big_init, dim3((unsigned)(((size_t)nbm * nbm + 255) / 256), W), dim3(256), 0, st, dD, dC); });
    launch_big_ldlt<false>(
        KT, KC_LDLT, B, W, st, ntm, n, [&](int k) { return 1 + (nbm - (k + 1) * kNB + 255) / 256; },
        [&](int k) { return (ntm - k - 1) * (ntm - k) / 2; });
  }
  if (sparse_trial) {  // the tile-sparse LDL^T: assembly into the pool, then the planned tiles' panels
    const int nw = cls_first[4] - cls_first[3];
    const unsigned ga = (unsigned)std::min<size_t>(16384, std::max<size_t>(1, (G.sp_elems + 255) / 256));
    KT.launch(KC_ASSEMBLE, [&] { hipLaunchKernelGGL(k_lba_assemble_tiles, dim3(ga, nw), dim3(256), 0, st, dD, dC, dO, dWins + cls_first[3]); });
    launch_big_ldlt<true>(
        KT, KC_LDLT_SPARSE, B, W, st, G.sp_nt, cls_max[3], [&](int k) { return G.sp_panel_grid[k]; },
        [&](int k) { return G.sp_syrk_grid[k]; });
  }
  if (cls_max[0] > 0 && cls_trial[0])
    KT.launch(KC_LDLT, [&] { hipLaunchKernelGGL(k_lba_ldlt16<kLd16Threads>, dim3(W), dim3(kLd16Threads), ld16_lds_bytes(G.nb16), st, dD, dC, dO, G.nb16); });
  if (cls_max[1] > 0 && cls_trial[1])
    KT.launch(KC_LDLT, [&] { hipLaunchKernelGGL(k_lba_ldltg<kLdGThreads>, dim3(W), dim3(kLdGThreads), ldg_lds_bytes(G.nbg), st, dD, dC, dO, G.nbg); });
  if (G.fused_tail)
    KT.launch(KC_UPDATE, [&] { hipLaunchKernelGGL(k_lba_tail, dim3(gq + max_imu, W), dim3(256), 0, st, dD, dC, dO, gq); });
  else {
    KT.launch(KC_UPDATE, [&] { hipLaunchKernelGGL(k_lba_update_points, dim3(gq, W), dim3(256), 0, st, dD, dC, dO); });
    KT.launch(KC_ERROR, [&] { hipLaunchKernelGGL(k_lba_error, dim3(ge, W), dim3(256), 0, st, dD, dC, 1); });
    if (max_imu > 0) KT.launch(KC_GENERIC, [&] { hipLaunchKernelGGL(k_lba_generic, dim3(max_imu, W), dim3(64), 0, st, dD, dC, 1); });
    KT.launch(KC_OTHER, [&] { hipLaunchKernelGGL(k_lba_reduce, dim3(W), dim3(256), 0, st, dD, dC, dO); });
  }
  if (sh) {  // chi2 and the landmark part of the gain-ratio scale
    if ((rc = shard_exchange(sh, sh->d_buf + G.shard_sys, 4 * (size_t)W, st)) != VIEO_OK) return rc;
    VIEO_HIP_CHECK(hipMemcpyAsync(B.h_sc, sh->d_buf + G.shard_sys, 32 * (size_t)W, hipMemcpyDeviceToHost, st));
  }
  VIEO_HIP_CHECK(hipMemcpyAsync(B.out, dO, (size_t)W * sizeof(WinOut), hipMemcpyDeviceToHost, st));
  return VIEO_OK;
}

// Results of the windows that took part, from the staging copy `hs` of the arena's result region.
static void lba_write_back(const LbaCall& c, std::vector<WinHost>& win, const uint8_t* hs) {
  const bool vio = c.vio();
  for (int w = 0; w < c.W; w++) {
    WinHost& H = win[w];
    if (H.skip) continue;
    vieo_lba_result* R = H.lm.R;
    if (vio) {  // float err / err_end and the divergence guard (Optimizer.cc:531-533,655-666)
      const float err = (float)R->chi2_initial, err_end = (float)H.lm.lastTrialChi;
      R->chi2_initial = err, R->chi2_final = err_end;
      if ((2 * err < err_end || std::isnan(err) || std::isnan(err_end)) && !H.VP->large && !c.gba) {
        R->status = VIEO_LBA_DIVERGED;
        continue;  // returns without write-back: outputs stay equal to the inputs
      }
    }
    if (H.n_obs > 0) memcpy(c.h_erase[w], hs + H.o_erase, H.n_obs);
    for (int i = 0; i < H.n_obs; i++) R->n_erase += c.h_erase[w][i];
    const LbaKf* o = (const LbaKf*)(hs + H.o_kf);
    const double* X = (const double*)(hs + H.o_X);
    vieo_navstate* navs = c.h_navs_out[w];
    for (int k = 0; k < H.n_kf; k++) {
      if (c.h_kfs[w][k].fixed) continue;
      memcpy(navs[k].p, o[k].p, 24);
      navs[k].q[0] = o[k].qw, navs[k].q[1] = o[k].qx, navs[k].q[2] = o[k].qy, navs[k].q[3] = o[k].qz;
      if (vio) {  // ns_recov: v of the V vertex, dbg / dba of the Bias vertex (Optimizer.cc:716-733)
        memcpy(navs[k].v, o[k].v, 24);
        memcpy(navs[k].dbg, o[k].dbg, 24), memcpy(navs[k].dba, o[k].dba, 24);
      }
    }
    float* pts = c.h_points_out[w];
    if (c.sco()) {  // SetWorldPos(scale * vPoint->estimate().cast<float>()) (Optimizer.cc:1321): a float product
      const double scale = *(const double*)(hs + H.o_scl);
      const float sf = (float)scale;
      for (int i = 0; i < H.n_mp * 3; i++) pts[i] = sf * (float)X[i];
      if (c.gba->scale_out) *c.gba->scale_out = scale;
    } else
      for (int i = 0; i < H.n_mp * 3; i++) pts[i] = (float)X[i];  // SetWorldPos(cast<float>)
  }
}

static int lba_run(const LbaCall& c) {
  const LbaShard* sh = c.sh;
  const int W = c.W;
  if (c.gba && c.gba->scale_out) *c.gba->scale_out = 1.0;
  bool shard_stop = false;  // a sharded run's collective view of the stop flag (latched)
  int rc = lba_check_and_agree(c, &shard_stop);
  if (rc != VIEO_OK) return rc;
  ShardStagingGuard staging_guard{sh};  // from here to the second agreement every early return reports to the other ranks
  hipStream_t st;
  if ((rc = lba_stream(&st)) != VIEO_OK) return rc;
  // VIEO_LBA_TIMING=1: host phases of a call on stderr (staging, rounds, results)
  static const bool host_timing = getenv("VIEO_LBA_TIMING") != nullptr;
  const auto t_enter = std::chrono::steady_clock::now();
  auto ms_since = [](std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
  };
  std::vector<WinHost> win(W);
  if (!lba_open_windows(c, sh ? shard_stop : c.stop_raised(), win)) {
    staging_guard.done = true;  // (key frames and stop state are replicated: the ranks of a sharded run all leave here together)
    return VIEO_OK;
  }
  std::vector<LbaDev> devs(W);
  LbaLayout L;
  LbaGrids G;
  lba_layout(c, win, devs, L, G);
  if ((rc = g_stage.ensure(L.res_end)) != VIEO_OK) return rc;
  uint8_t* hs = (uint8_t*)g_stage.p;
  const double ms_layout = ms_since(t_enter);
  if ((rc = lba_stage(c, win, devs, L, hs)) != VIEO_OK) return rc;
  const double ms_filled = ms_since(t_enter);
  if ((rc = lba_describe(c, win, devs, L, G)) != VIEO_OK) return rc;
  const LbaBufs B = lba_bufs(W);
  const double ms_described = ms_since(t_enter);
  if ((rc = lba_enqueue(c, L, devs, G, B, hs, st)) != VIEO_OK) return rc;
  if (sh) {  // second agreement: every rank staged its windows (ShardStagingGuard reports the ones that did not)
    VIEO_HIP_CHECK(hipStreamSynchronize(st));
    double sum = 1.0;
    staging_guard.done = true;
    const int xrc = shard_agree(sh, true, &sum);
    if (xrc != VIEO_OK) return xrc;
    if (sum != 0.0) {
      set_error("sharded local BA: another rank failed while staging its windows, all ranks return");
      return VIEO_E_INVALID;
    }
  }
  // ---- lock-step rounds: plan the round, launch it, wait, digest the trials
  const double ms_staged = ms_since(t_enter);
  const auto t_rounds = std::chrono::steady_clock::now();
  int n_rounds = 0;
  double ms_wait = 0;
  static thread_local LbaKTimer KT;
  KT.begin(st);
  const LmMode mode = c.lm_mode();
  for (;;) {
    n_rounds++;
    const bool stop_now = sh ? shard_stop : c.stop_raised();
    const int stop_req = sh && c.stop_raised() ? 1 : 0;  // (sharded: travels as ctl.pad -> the trial's fourth scalar)
    int any = 0;
    bool cls_trial[4] = {false, false, false, false};  // which solve kernels have a window this round
    for (int w = 0; w < W; w++) {
      B.ctl[w] = lm_plan_round(win[w].lm, mode, stop_now, stop_req);
      any |= B.ctl[w].flags;
      if ((B.ctl[w].flags & LBA_TRIAL) && !win[w].skip) cls_trial[win[w].cls] = true;
    }
    if (!any) break;
    if ((rc = launch_round(c, G, B, KT, any, cls_trial, st)) != VIEO_OK) return rc;
    VIEO_HIP_CHECK(hipGetLastError());
    {
      const auto t_w = std::chrono::steady_clock::now();
      VIEO_HIP_CHECK(hipStreamSynchronize(st));
      ms_wait += ms_since(t_w);
    }
    if (KT.on) {
      // the windows this round's k_lba_schur launch worked on: dense count 2 np (np + 1) 3 n_mp of the visual part of
      // a window's Schur complement
      double fl = 0;
      for (int w = 0; w < W; w++)
        if ((B.ctl[w].flags & LBA_TRIAL) && !win[w].skip)
          fl += 2.0 * (6 * devs[w].nf_cap) * (6 * devs[w].nf_cap + 1) * 3.0 * devs[w].n_mp;
      KT.fold(fl);
    }
    if (sh)  // the ranks' stop requests of this round (the same count in every window that ran a trial)
      for (int w = 0; w < W; w++)
        if (lm_shard_stop_requested(B.ctl[w].flags, B.h_sc + 4 * w)) shard_stop = true;
    for (int w = 0; w < W; w++)
      lm_digest_trial(win[w].lm, mode, B.ctl[w].flags, B.out[w], sh ? B.h_sc + 4 * w : nullptr,
                      sh ? shard_stop : c.stop_raised());
  }
  // ---- results: one copy for all windows
  const double ms_rounds = ms_since(t_rounds);
  const auto t_res = std::chrono::steady_clock::now();
  VIEO_HIP_CHECK(hipMemcpyAsync(hs + L.res_begin, g_arena.as<uint8_t>() + L.res_begin, L.res_end - L.res_begin,
                                hipMemcpyDeviceToHost, st));
  VIEO_HIP_CHECK(hipStreamSynchronize(st));
  if (host_timing)
    fprintf(stderr, "lba_run: %d windows, staging %.3f ms, %d rounds %.3f ms (of which waiting for the stream %.3f), "
                    "results copy %.3f ms; staging: layout %.3f, windows filled %.3f, descriptors %.3f, enqueued %.3f\n", W, ms_staged,
            n_rounds, ms_rounds, ms_wait, ms_since(t_res), ms_layout, ms_filled, ms_described, ms_staged);
  lba_write_back(c, win, hs);
  return VIEO_OK;
}

}  // namespace vieo

using namespace vieo;

// a full BA has no erase flags to return: one window, with a throw-away array in their place
static int gba_run(LbaCall& c, const GbaMode& g, int n_obs) {
  std::vector<uint8_t> erase((size_t)std::max(n_obs, 1));
  uint8_t* er = erase.data();
  c.gba = &g, c.W = 1, c.h_erase = &er;
  return lba_run(c);
}

extern "C" {

int vieo_lba_set_stream_priority(int priority) {
  if (priority < -1 || priority > 1) return VIEO_E_INVALID;
  if (priority != g_lba_priority && g_lba_stream) {  // the next call creates the stream again
    (void)hipStreamSynchronize(g_lba_stream);
    (void)hipStreamDestroy(g_lba_stream);
    g_lba_stream = nullptr;
  }
  g_lba_priority = priority;
  return VIEO_OK;
}

int vieo_local_bundle_adjustment_batch_enc(int n_windows, const vieo_lba_params* const* params,
                                           const vieo_lba_keyframe* const* h_kfs, const int* n_kf,
                                           const float* const* h_points, const int* n_mp,
                                           const vieo_lba_obs* const* h_obs, const int* n_obs,
                                           const vieo_lba_enc* const* encs, volatile const int* stop,
                                           vieo_navstate* const* h_navs_out, float* const* h_points_out,
                                           uint8_t* const* h_erase, vieo_lba_result* h_results) {
  LbaCall c;
  c.W = n_windows, c.params = params, c.encs = encs;
  c.h_kfs = h_kfs, c.n_kf = n_kf, c.h_points = h_points, c.n_mp = n_mp, c.h_obs = h_obs, c.n_obs = n_obs;
  c.stop = stop;
  c.h_navs_out = h_navs_out, c.h_points_out = h_points_out, c.h_erase = h_erase, c.h_results = h_results;
  return lba_run(c);
}

int vieo_local_bundle_adjustment_batch(int n_windows, const vieo_lba_params* const* params,
                                       const vieo_lba_keyframe* const* h_kfs, const int* n_kf,
                                       const float* const* h_points, const int* n_mp,
                                       const vieo_lba_obs* const* h_obs, const int* n_obs,
                                       volatile const int* stop, vieo_navstate* const* h_navs_out,
                                       float* const* h_points_out, uint8_t* const* h_erase,
                                       vieo_lba_result* h_results) {
  return vieo_local_bundle_adjustment_batch_enc(n_windows, params, h_kfs, n_kf, h_points, n_mp, h_obs, n_obs, nullptr, stop,
                                                h_navs_out, h_points_out, h_erase, h_results);
}

int vieo_local_bundle_adjustment(const vieo_lba_params* P, const vieo_lba_keyframe* h_kfs, int n_kf,
                                 const float* h_points, int n_mp, const vieo_lba_obs* h_obs, int n_obs,
                                 volatile const int* stop, vieo_navstate* h_navs_out,
                                 float* h_points_out, uint8_t* h_erase, vieo_lba_result* R) {
  return vieo_local_bundle_adjustment_enc(P, h_kfs, n_kf, h_points, n_mp, h_obs, n_obs, nullptr, stop, h_navs_out, h_points_out,
                                          h_erase, R);
}

int vieo_local_bundle_adjustment_enc(const vieo_lba_params* P, const vieo_lba_keyframe* h_kfs, int n_kf,
                                     const float* h_points, int n_mp, const vieo_lba_obs* h_obs, int n_obs,
                                     const vieo_lba_enc* enc, volatile const int* stop, vieo_navstate* h_navs_out,
                                     float* h_points_out, uint8_t* h_erase, vieo_lba_result* R) {
  if (!P || !h_kfs || n_kf <= 0 || !h_points || n_mp <= 0 || !h_obs || n_obs <= 0 || !h_navs_out ||
      !h_points_out || !h_erase || !R)
    return VIEO_E_INVALID;
  return vieo_local_bundle_adjustment_batch_enc(1, &P, &h_kfs, &n_kf, &h_points, &n_mp, &h_obs, &n_obs, &enc, stop,
                                                &h_navs_out, &h_points_out, &h_erase, R);
}

int vieo_bundle_adjustment_enc(const vieo_lba_params* params, int n_iterations, int robust,
                               const vieo_lba_keyframe* h_kfs, int n_kf, const float* h_points, int n_mp,
                               const vieo_lba_obs* h_obs, int n_obs, const vieo_lba_enc* enc,
                               volatile const int* stop, vieo_navstate* h_navs_out, float* h_points_out,
                               vieo_lba_result* h_result) {
  if (!params || n_iterations < 0 || !h_result || n_obs < 0) return VIEO_E_INVALID;
  const GbaMode g = {n_iterations, robust};
  LbaCall c;
  c.params = &params, c.encs = &enc;
  c.h_kfs = &h_kfs, c.n_kf = &n_kf, c.h_points = &h_points, c.n_mp = &n_mp, c.h_obs = &h_obs, c.n_obs = &n_obs;
  c.stop = stop;
  c.h_navs_out = &h_navs_out, c.h_points_out = &h_points_out, c.h_results = h_result;
  return gba_run(c, g, n_obs);
}

int vieo_bundle_adjustment(const vieo_lba_params* params, int n_iterations, int robust,
                           const vieo_lba_keyframe* h_kfs, int n_kf, const float* h_points, int n_mp,
                           const vieo_lba_obs* h_obs, int n_obs, volatile const int* stop, vieo_navstate* h_navs_out,
                           float* h_points_out, vieo_lba_result* h_result) {
  return vieo_bundle_adjustment_enc(params, n_iterations, robust, h_kfs, n_kf, h_points, n_mp, h_obs, n_obs, nullptr, stop,
                                    h_navs_out, h_points_out, h_result);
}

int vieo_local_bundle_adjustment_vio_batch(int n_windows, const vieo_lba_vio_params* const* params,
                                           const vieo_lba_keyframe* const* h_kfs, const int* n_kf,
                                           const float* const* h_points, const uint8_t* const* h_close,
                                           const int* n_mp, const vieo_lba_obs* const* h_obs, const int* n_obs,
                                           const vieo_lba_imu_edge* const* h_imu, const int* n_imu,
                                           volatile const int* stop, vieo_navstate* const* h_navs_out,
                                           float* const* h_points_out, uint8_t* const* h_erase,
                                           vieo_lba_result* h_results) {
  if (!params) return VIEO_E_INVALID;
  LbaCall c;
  c.W = n_windows, c.vparams = params;
  c.h_kfs = h_kfs, c.n_kf = n_kf, c.h_points = h_points, c.h_close = h_close, c.n_mp = n_mp;
  c.h_obs = h_obs, c.n_obs = n_obs, c.h_imu = h_imu, c.n_imu = n_imu;
  c.stop = stop;
  c.h_navs_out = h_navs_out, c.h_points_out = h_points_out, c.h_erase = h_erase, c.h_results = h_results;
  return lba_run(c);
}

int vieo_local_bundle_adjustment_vio(const vieo_lba_vio_params* P, const vieo_lba_keyframe* h_kfs, int n_kf,
                                     const float* h_points, const uint8_t* h_close, int n_mp,
                                     const vieo_lba_obs* h_obs, int n_obs, const vieo_lba_imu_edge* h_imu,
                                     int n_imu, volatile const int* stop, vieo_navstate* h_navs_out,
                                     float* h_points_out, uint8_t* h_erase, vieo_lba_result* R) {
  if (!P || !h_kfs || n_kf <= 0 || !h_points || !h_close || n_mp <= 0 || !h_obs || n_obs <= 0 || n_imu < 0 ||
      (n_imu > 0 && !h_imu) || !h_navs_out || !h_points_out || !h_erase || !R)
    return VIEO_E_INVALID;
  return vieo_local_bundle_adjustment_vio_batch(1, &P, &h_kfs, &n_kf, &h_points, &h_close, &n_mp, &h_obs, &n_obs,
                                                &h_imu, &n_imu, stop, &h_navs_out, &h_points_out, &h_erase, R);
}

size_t vieo_lba_sharded_buffer_doubles(int n_windows, const int* n_free_kf) {
  size_t n = 0;
  for (int w = 0; w < n_windows; w++) n += shard_sys_doubles(n_free_kf ? n_free_kf[w] : 0, 1) + 4;  // (room for the scale vertex)
  return n;
}

int vieo_local_bundle_adjustment_vio_sharded_stop(int n_windows, const vieo_lba_vio_params* const* params,
                                                  const vieo_lba_keyframe* const* h_kfs, const int* n_kf,
                                                  const float* const* h_points, const uint8_t* const* h_close,
                                                  const int* n_mp, const vieo_lba_obs* const* h_obs, const int* n_obs,
                                                  const vieo_lba_imu_edge* const* h_imu, const int* n_imu,
                                                  double* d_reduce_buf, size_t reduce_cap_doubles,
                                                  vieo_allreduce_sum_f64_fn allreduce, void* ctx, volatile const int* stop,
                                                  vieo_navstate* const* h_navs_out, float* const* h_points_out,
                                                  uint8_t* const* h_erase, vieo_lba_result* h_results) {
  if (!params) return VIEO_E_INVALID;
  const LbaShard sh{allreduce, ctx, d_reduce_buf, reduce_cap_doubles};
  LbaCall c;
  c.sh = &sh;
  c.W = n_windows, c.vparams = params;
  c.h_kfs = h_kfs, c.n_kf = n_kf, c.h_points = h_points, c.h_close = h_close, c.n_mp = n_mp;
  c.h_obs = h_obs, c.n_obs = n_obs, c.h_imu = h_imu, c.n_imu = n_imu;
  c.stop = stop;
  c.h_navs_out = h_navs_out, c.h_points_out = h_points_out, c.h_erase = h_erase, c.h_results = h_results;
  return lba_run(c);
}

int vieo_local_bundle_adjustment_vio_sharded(int n_windows, const vieo_lba_vio_params* const* params,
                                             const vieo_lba_keyframe* const* h_kfs, const int* n_kf,
                                             const float* const* h_points, const uint8_t* const* h_close,
                                             const int* n_mp, const vieo_lba_obs* const* h_obs, const int* n_obs,
                                             const vieo_lba_imu_edge* const* h_imu, const int* n_imu,
                                             double* d_reduce_buf, size_t reduce_cap_doubles,
                                             vieo_allreduce_sum_f64_fn allreduce, void* ctx,
                                             vieo_navstate* const* h_navs_out, float* const* h_points_out,
                                             uint8_t* const* h_erase, vieo_lba_result* h_results) {
  return vieo_local_bundle_adjustment_vio_sharded_stop(n_windows, params, h_kfs, n_kf, h_points, h_close, n_mp, h_obs, n_obs, h_imu,
                                                       n_imu, d_reduce_buf, reduce_cap_doubles, allreduce, ctx, nullptr, h_navs_out,
                                                       h_points_out, h_erase, h_results);
}

// the visual-inertial full BAs: sh == nullptr, or one rank of a landmark-sharded run
static int gba_vio_run(const LbaShard* sh, const vieo_lba_vio_params* params, int n_iterations, int robust, int scale_opt,
                       const vieo_lba_keyframe* h_kfs, int n_kf, const float* h_points, int n_mp,
                       const vieo_lba_obs* h_obs, int n_obs, const vieo_lba_imu_edge* h_imu, int n_imu,
                       volatile const int* stop, vieo_navstate* h_navs_out, float* h_points_out,
                       vieo_lba_result* h_result, double* h_scale_out) {
  if (!params || n_iterations < 0 || !h_result || n_obs < 0) return VIEO_E_INVALID;
  GbaMode g = {n_iterations, robust};
  g.scale_opt = scale_opt != 0, g.scale_out = h_scale_out;
  const uint8_t* no_close = nullptr;
  LbaCall c;
  c.sh = sh;
  c.vparams = &params;
  c.h_kfs = &h_kfs, c.n_kf = &n_kf, c.h_points = &h_points, c.h_close = &no_close, c.n_mp = &n_mp;
  c.h_obs = &h_obs, c.n_obs = &n_obs, c.h_imu = &h_imu, c.n_imu = &n_imu;
  c.stop = stop;
  c.h_navs_out = &h_navs_out, c.h_points_out = &h_points_out, c.h_results = h_result;
  return gba_run(c, g, n_obs);
}

int vieo_global_bundle_adjustment_vio_sharded_scale(const vieo_lba_vio_params* params, int n_iterations, int robust,
                                                    int scale_opt, const vieo_lba_keyframe* h_kfs, int n_kf,
                                                    const float* h_points, int n_mp, const vieo_lba_obs* h_obs, int n_obs,
                                                    const vieo_lba_imu_edge* h_imu, int n_imu, double* d_reduce_buf,
                                                    size_t reduce_cap_doubles, vieo_allreduce_sum_f64_fn allreduce,
                                                    void* ctx, vieo_navstate* h_navs_out, float* h_points_out,
                                                    vieo_lba_result* h_result, double* h_scale_out) {
  const LbaShard sh{allreduce, ctx, d_reduce_buf, reduce_cap_doubles};
  return gba_vio_run(&sh, params, n_iterations, robust, scale_opt, h_kfs, n_kf, h_points, n_mp, h_obs, n_obs, h_imu, n_imu,
                     nullptr, h_navs_out, h_points_out, h_result, h_scale_out);
}

int vieo_global_bundle_adjustment_vio_sharded(const vieo_lba_vio_params* params, int n_iterations, int robust,
                                              const vieo_lba_keyframe* h_kfs, int n_kf, const float* h_points,
                                              int n_mp, const vieo_lba_obs* h_obs, int n_obs,
                                              const vieo_lba_imu_edge* h_imu, int n_imu, double* d_reduce_buf,
                                              size_t reduce_cap_doubles, vieo_allreduce_sum_f64_fn allreduce,
                                              void* ctx, vieo_navstate* h_navs_out, float* h_points_out,
                                              vieo_lba_result* h_result) {
  return vieo_global_bundle_adjustment_vio_sharded_scale(params, n_iterations, robust, 0, h_kfs, n_kf, h_points, n_mp,
                                                         h_obs, n_obs, h_imu, n_imu, d_reduce_buf, reduce_cap_doubles,
                                                         allreduce, ctx, h_navs_out, h_points_out, h_result, nullptr);
}

int vieo_global_bundle_adjustment_vio_scale(const vieo_lba_vio_params* params, int n_iterations, int robust, int scale_opt,
                                            const vieo_lba_keyframe* h_kfs, int n_kf, const float* h_points, int n_mp,
                                            const vieo_lba_obs* h_obs, int n_obs, const vieo_lba_imu_edge* h_imu,
                                            int n_imu, volatile const int* stop, vieo_navstate* h_navs_out,
                                            float* h_points_out, vieo_lba_result* h_result, double* h_scale_out) {
  return gba_vio_run(nullptr, params, n_iterations, robust, scale_opt, h_kfs, n_kf, h_points, n_mp, h_obs, n_obs, h_imu, n_imu,
                     stop, h_navs_out, h_points_out, h_result, h_scale_out);
}

int vieo_global_bundle_adjustment_vio(const vieo_lba_vio_params* params, int n_iterations, int robust,
                                      const vieo_lba_keyframe* h_kfs, int n_kf, const float* h_points, int n_mp,
                                      const vieo_lba_obs* h_obs, int n_obs, const vieo_lba_imu_edge* h_imu, int n_imu,
                                      volatile const int* stop, vieo_navstate* h_navs_out, float* h_points_out,
                                      vieo_lba_result* h_result) {
  return vieo_global_bundle_adjustment_vio_scale(params, n_iterations, robust, 0, h_kfs, n_kf, h_points, n_mp, h_obs, n_obs,
                                                 h_imu, n_imu, stop, h_navs_out, h_points_out, h_result, nullptr);
}

// Kernel-class timing of the bundle-adjustment engine (bench.py's roofline over the whole path).
void vieo_lba_enable_timing(int on) {
  std::lock_guard<std::mutex> g(vieo::g_lba_kt_mutex);
  vieo::g_lba_ktiming.store(on == 2 ? 2 : (on ? 1 : 0));
  for (int i = 0; i < vieo::KC_N; i++) vieo::g_lba_kt_ms[i] = 0, vieo::g_lba_kt_launches[i] = 0;
  vieo::g_lba_kt_schur_flops = 0;
}
int vieo_lba_kernel_classes(void) { return vieo::KC_N; }
const char* vieo_lba_kernel_class_name(int i) { return i >= 0 && i < vieo::KC_N ? vieo::kLbaKClassName[i] : ""; }
void vieo_lba_kernel_times(double* ms, long long* launches, double* schur_flops) {
  std::lock_guard<std::mutex> g(vieo::g_lba_kt_mutex);
  for (int i = 0; i < vieo::KC_N; i++) ms[i] = vieo::g_lba_kt_ms[i], launches[i] = vieo::g_lba_kt_launches[i];
  *schur_flops = vieo::g_lba_kt_schur_flops;
}
void vieo_lba_sparse_stats(long long* out) {
  std::lock_guard<std::mutex> g(vieo::g_lba_kt_mutex);
  for (int i = 0; i < 6; i++) out[i] = vieo::g_lba_sparse_stats[i];
}
}  // extern "C"
