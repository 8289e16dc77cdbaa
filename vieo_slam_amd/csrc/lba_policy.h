// lba_policy.h -- the Levenberg-Marquardt policy of the lock-step bundle-adjustment driver (lba.hip): which steps a
// window takes in the next round and what a finished trial means for it.  Host arithmetic only, exactly g2o's
// (optimization_algorithm_levenberg.cpp:61-164 inside sparse_optimizer's iteration loop) under the two-stage
// optimize(its0) -> classify -> optimize(its1) -> classify of Optimizer::LocalBundleAdjustment; no HIP in here, so
// that tests/test_lba_policy.py drives it on the CPU.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "../../include/vieo_hot.h"

#ifdef __HIPCC__
#define VIEO_LM_HD __host__ __device__ inline
#else
#define VIEO_LM_HD inline
#endif

namespace vieo {

// ---- the arithmetic of the policy, host and device: the drivers below run it on the host from one record per round,
// the Sim3 optimisation of loop verification (sim3_optimize_device.h) runs it inside its kernel.
struct LmCore {
  double lambda = -1, ni = 2, currentChi = 0, iniChi = 0;
  int nBad = 0, qmax = 0, it = 0;
};

// One lambda trial is evaluated (optimization_algorithm_levenberg.cpp:126-148): ok2 = the factorisation succeeded, chi2 =
// activeRobustChi2 at the trial state, scale_sum = computeScale().  Returns rho; *accepted: the state is kept.
VIEO_LM_HD double lm_core_trial(LmCore& c, bool ok2, double chi2, double scale_sum, bool* accepted) {
  const double tempChi = ok2 ? chi2 : DBL_MAX;
  double rho = c.currentChi - tempChi;
  const double scale = (ok2 ? scale_sum : 0.0) + 1e-3;
  rho /= scale;
  *accepted = rho > 0 && fabs(tempChi) <= DBL_MAX;  // g2o_isfinite
  if (*accepted) {
    double alpha = 1. - pow(2 * rho - 1, 3.0);
    alpha = 2. / 3. < alpha ? 2. / 3. : alpha;   // std::min(alpha, _goodStepUpperScale)
    c.lambda *= 1. / 3. < alpha ? alpha : 1. / 3.;  // std::max(_goodStepLowerScale, alpha)
    c.ni = 2;
    c.currentChi = tempChi;
  } else {
    c.lambda *= c.ni;
    c.ni *= 2;
  }
  c.qmax++;
  return rho;
}

// The trials of an iteration are over (:151-163 and the loop of SparseOptimizer::optimize): true when the optimize() is
// over too, otherwise the next iteration starts at the accepted state.
VIEO_LM_HD bool lm_core_iteration_end(LmCore& c, double rho, int iters, bool stopped) {
  bool terminate = c.qmax == 10 || rho == 0;
  if (!terminate) {
    if ((c.iniChi - c.currentChi) * 1e3 < c.iniChi)
      c.nBad++;
    else
      c.nBad = 0;
    terminate = c.nBad >= 3;
  }
  c.it++;
  if (terminate || c.it >= iters || stopped) return true;
  c.iniChi = c.currentChi;
  c.qmax = 0;
  return false;
}

// control word of a window for one round of the lock-step driver
enum {
  LBA_TRIAL = 1,    // solve + update + evaluate one lambda trial
  LBA_BUILD = 2,    // re-linearise (start of an LM iteration)
  LBA_RESTORE = 4,  // the last trial was rejected: restore the backed-up estimates first
  LBA_BEGIN = 8,    // start of an optimize(): active sets, initial chi2, lambda init
  LBA_CLASS0 = 16,  // chi2 / depth gates -> level 1 (between the two optimisations)
  LBA_CLASS1 = 32,  // final erase flags
  LBA_ROBUST = 64,  // Huber kernels on (first optimisation)
  LBA_PRELEVEL = 128,  // GraphOperator::Chi2LargeSetLevel before the first optimisation (a18)
};
struct WinCtl {
  int flags, pad;
  double lambda;  // < 0: take the device-computed initial lambda
};
struct WinOut {
  double chi0, chi2, scale_l, scale_p, lambda;
  int ok, np;
  double chig0, chig;  // landmark-sharded windows: the (replicated) inertial part, kept out of the reduction
};

struct LmMode {  // what a call fixes for all its windows
  bool full_ba = false;    // Optimizer::BundleAdjustment: ONE optimize(), no classification, no Chi2LargeSetLevel
  bool robust = false;     // full BA: Huber kernels on every edge (a local BA has them in its first optimize() only)
  bool vio_local = false;  // visual-inertial local BA: setUserLambdaInit(lambda_init), Chi2LargeSetLevel once
  bool user_lambda = false;  // setUserLambdaInit(lambda_init) alone (the pose graph of pose_graph.hip)
};

struct WinLm : LmCore {  // per-window LM state machine
  vieo_lba_result* R = nullptr;
  int its1 = 0;              // iterations of the second optimize()
  double lambda_init = 0;    // vio_local / user_lambda: setUserLambdaInit (Optimizer.cc:131-138, :2333)
  double lastTrialChi = 0;   // activeRobustChi2 of the errors left in the edges (err_end)
  bool prelevel_pending = false;
  int stage = 0;  // 0: optimize(its0), 1: optimize(its1), 2: finished
  int phase = 0;  // 0: the next round starts an optimize(), 1: in trials, 2: optimize() is over
  int iters = 0;
  bool need_build = false, need_restore = false;
};

// its0: iterations of the first optimize() (the full BA's only one)
inline void lm_start(WinLm& H, const LmMode& m, int its0, int its1, double lambda_init, vieo_lba_result* R) {
  H = WinLm();
  H.R = R, H.its1 = its1, H.lambda_init = lambda_init;
  H.prelevel_pending = m.vio_local;
  H.iters = its0;
  H.phase = H.iters > 0 ? 0 : 2;
}

// a window that takes no part in the rounds (no free pose, stop flag raised before the call)
inline void lm_skip(WinLm& H, int status) { H.R->status = status, H.stage = 2; }

// The window's control word and lambda for the next round.  stop_now: the stop flag as the driver sees it at the start of
// the round; pad travels to the device unchanged (a sharded run's own stop request).  flags == 0: the window is finished.
inline WinCtl lm_plan_round(WinLm& H, const LmMode& m, bool stop_now, int pad) {
  int f = 0;
  double lam = H.lambda;
  if (H.stage < 2 && H.phase == 2) {  // an optimize() is over
    if (H.need_restore) f |= LBA_RESTORE, H.need_restore = false;
    if (m.full_ba)
      H.stage = 2;
    else if (H.stage == 0 && !stop_now) {
      f |= LBA_CLASS0;
      H.stage = 1, H.iters = H.its1, H.phase = H.iters > 0 ? 0 : 2;
    } else {
      if (H.stage == 0) H.R->status = VIEO_LBA_ABORTED;  // stop flag between the two stages
      f |= LBA_CLASS1;
      H.stage = 2;
    }
  }
  const int robust = (m.full_ba ? m.robust : H.stage == 0) ? LBA_ROBUST : 0;
  if (H.stage < 2 && H.phase == 0) {
    f |= LBA_BEGIN | LBA_BUILD | LBA_TRIAL | robust;
    lam = m.vio_local || m.user_lambda ? H.lambda_init : -1;
    if (H.prelevel_pending) f |= LBA_PRELEVEL, H.prelevel_pending = false;
  } else if (H.stage < 2 && H.phase == 1) {
    f |= LBA_TRIAL | robust;
    if (H.need_build) f |= LBA_BUILD;
    if (H.need_restore) f |= LBA_RESTORE, H.need_restore = false;
  }
  return WinCtl{f, pad, lam};
}

// sc: the four reduced scalars of a window of a landmark-sharded run [chi0, chi2, scale_l, stop requests]
inline bool lm_shard_stop_requested(int flags, const double* sc) { return (flags & (LBA_TRIAL | LBA_BEGIN)) && sc[3] > 0; }

// What the trial of a round (flags: its control word) means for the window.  sc != nullptr: a sharded run -- the totals
// are all ranks' visual edges (sc) + the replicated inertial edges (chig0 / chig), written into `out`.  stopped: the
// stop flag as the driver sees it now.
inline void lm_digest_trial(WinLm& H, const LmMode& m, int flags, WinOut& out, const double* sc, bool stopped) {
  if (!(flags & LBA_TRIAL)) return;
  if (sc) out.chi0 = sc[0] + out.chig0, out.chi2 = sc[1] + out.chig, out.scale_l = sc[2];
  if (flags & LBA_BEGIN) {
    if (out.np == 0) {  // no active free vertex: optimize() returns at once
      H.phase = 2;
      return;
    }
    H.R->lm_iterations++;
    H.currentChi = out.chi0;
    if (H.stage == 0) H.R->chi2_initial = H.currentChi;
    H.iniChi = H.currentChi;
    H.lambda = m.vio_local || m.user_lambda ? H.lambda_init : out.lambda;
    H.ni = 2, H.nBad = 0, H.qmax = 0, H.it = 0;
    H.phase = 1;
  }
  H.R->lm_trials++;
  H.need_build = false;
  H.lastTrialChi = out.chi2;
  bool accepted;
  const double rho = lm_core_trial(H, out.ok != 0, out.chi2, out.scale_l + out.scale_p, &accepted);
  if (!accepted) H.need_restore = true;
  H.R->chi2_final = H.currentChi;
  if (rho < 0 && H.qmax < 10 && !stopped) return;  // next lambda trial of the same iteration
  if (lm_core_iteration_end(H, rho, H.iters, stopped))
    H.phase = 2;
  else {
    H.R->lm_iterations++;
    H.need_build = true;  // buildSystem at the accepted state
  }
}

}  // namespace vieo
