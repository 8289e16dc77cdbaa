"""The host-side Levenberg-Marquardt policy of the bundle-adjustment driver (vieo_slam_amd/csrc/lba_policy.h) against a
Python restatement of what the reference runs: Optimizer::LocalBundleAdjustment's optimize(its0) -> classify ->
optimize(its1) -> classify (one optimize() in the full BA), inside an optimize() g2o's iteration loop
(SparseOptimizer::optimize) around the up-to-10 lambda trials of OptimizationAlgorithmLevenberg::solve.  The driver
unrolls those loops into lock-step rounds; the test feeds both the same scripted trial outcomes (WinOut records) and
compares, round by round, the control word and the lambda, then the result record.  CPU only: the header is compiled
with g++ into a small library here."""
import ctypes
import math
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIAL, BUILD, RESTORE, BEGIN, CLASS0, CLASS1, ROBUST, PRELEVEL = 1, 2, 4, 8, 16, 32, 64, 128
OK, ABORTED, NO_FREE_POSE = 0, 1, 2
DBL_MAX = sys.float_info.max

_SHIM = r"""
#include "lba_policy.h"
using namespace vieo;
static WinLm g_lm;
static LmMode g_mode;
static vieo_lba_result g_res;
extern "C" void pol_start(int full_ba, int robust, int vio_local, int its0, int its1, double lambda_init) {
  g_mode.full_ba = full_ba != 0, g_mode.robust = robust != 0, g_mode.vio_local = vio_local != 0;
  g_res = vieo_lba_result();
  lm_start(g_lm, g_mode, its0, its1, lambda_init, &g_res);
}
extern "C" void pol_skip(int status) { lm_skip(g_lm, status); }
extern "C" void pol_plan(int stop_now, int pad, int* flags_pad, double* lambda) {
  const WinCtl c = lm_plan_round(g_lm, g_mode, stop_now != 0, pad);
  flags_pad[0] = c.flags, flags_pad[1] = c.pad, *lambda = c.lambda;
}
// o: chi0, chi2, scale_l, scale_p, lambda, ok, np, chig0, chig (the totals come back in o[0..2]); sc: 4 scalars or null
extern "C" void pol_digest(int flags, double* o, const double* sc, int stopped) {
  WinOut w = {o[0], o[1], o[2], o[3], o[4], (int)o[5], (int)o[6], o[7], o[8]};
  lm_digest_trial(g_lm, g_mode, flags, w, sc, stopped != 0);
  o[0] = w.chi0, o[1] = w.chi2, o[2] = w.scale_l;
}
extern "C" int pol_shard_stop(int flags, const double* sc) { return lm_shard_stop_requested(flags, sc) ? 1 : 0; }
extern "C" void pol_result(int* i, double* d) {
  i[0] = g_res.status, i[1] = g_res.lm_iterations, i[2] = g_res.lm_trials, i[3] = g_res.n_erase;
  d[0] = g_res.chi2_initial, d[1] = g_res.chi2_final;
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("lba_policy")
    src, so = d / "shim.cc", d / "liblbapolicy.so"
    src.write_text(_SHIM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC",
                           "-I" + os.path.join(ROOT, "vieo_slam_amd", "csrc"), str(src), "-o", str(so)])
    L = ctypes.CDLL(str(so))
    L.pol_start.argtypes = [ctypes.c_int] * 5 + [ctypes.c_double]
    L.pol_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.pol_digest.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    L.pol_shard_stop.argtypes = [ctypes.c_int, ctypes.c_void_p]
    return L


def rec(chi2, chi0=100.0, scale_l=1.0, scale_p=1.0, lam=1e-3, ok=1, np_=12, chig0=0.0, chig=0.0, sc=None):
    """One trial as the device reports it (WinOut); sc: the four reduced scalars of a sharded run."""
    return dict(chi0=chi0, chi2=chi2, scale_l=scale_l, scale_p=scale_p, lam=lam, ok=ok, np=np_, chig0=chig0, chig=chig, sc=sc)


class Case:
    def __init__(self, script, its0=5, its1=10, full_ba=False, robust=False, vio_local=False, lambda_init=0.0,
                 stop_time=None, skip=None):
        """stop_time: the stop flag is up from this moment on -- the plan of round r is moment 2 r, the digest of its
        trial 2 r + 1 (None: never; a sharded script raises it through its fourth scalar instead).  skip: the window is
        left out at entry with this status."""
        self.script, self.its0, self.its1 = script, its0, its1
        self.full_ba, self.robust, self.vio_local, self.lambda_init = full_ba, robust, vio_local, lambda_init
        self.stop_time, self.skip = stop_time, skip
        self.sharded = any(r["sc"] is not None for r in script)


# ---------------------------------------------------------------------------------------------- the reference, as loops
def model(c):
    """(rounds [(flags, lambda sent)], result dict, records consumed)"""
    rounds, used = [], [0]
    res = dict(status=OK, lm_iterations=0, lm_trials=0, chi2_initial=0.0, chi2_final=0.0)
    s = dict(lam=-1.0, carry=0, prelevel=c.vio_local, shard_stop=False)
    if c.skip is not None:
        res["status"] = c.skip
        return rounds, res, 0

    def stop(t):
        return s["shard_stop"] if c.sharded else (c.stop_time is not None and t >= c.stop_time)

    def trial(flags, lam_sent):  # one lock-step round with a trial: what goes to the device, what comes back
        rounds.append((flags | s["carry"], lam_sent))
        s["carry"] = 0
        r = dict(c.script[used[0]])
        used[0] += 1
        if r["sc"] is not None:  # totals over the ranks + the replicated inertial part; the ranks' stop requests
            r["chi0"], r["chi2"], r["scale_l"] = r["sc"][0] + r["chig0"], r["sc"][1] + r["chig"], r["sc"][2]
            if r["sc"][3] > 0:
                s["shard_stop"] = True
        return r

    def optimize(iterations, robust):  # SparseOptimizer::optimize + OptimizationAlgorithmLevenberg::solve
        rb = ROBUST if robust else 0
        current = ni = n_bad = 0
        for i in range(iterations):
            if i > 0 and stop(2 * len(rounds) - 1):  # terminate() at the head of the loop
                break
            first = BUILD | (BEGIN if i == 0 else 0)  # buildSystem; initializeOptimization + computeLambdaInit
            if i == 0 and s["prelevel"]:
                first |= PRELEVEL
                s["prelevel"] = False
            qmax = 0
            while True:
                begin = bool(first & BEGIN)
                r = trial(TRIAL | rb | first, ((c.lambda_init if c.vio_local else -1.0) if begin else s["lam"]))
                first = 0
                if begin:
                    if r["np"] == 0:  # no vertex to optimise: optimize() returns at once
                        return
                    current = r["chi0"]
                    if first_optimize[0]:
                        res["chi2_initial"] = current
                    s["lam"] = c.lambda_init if c.vio_local else r["lam"]
                    ni, n_bad = 2.0, 0
                if qmax == 0:  # the first trial of solve(i)
                    res["lm_iterations"] += 1
                    ini = current
                res["lm_trials"] += 1
                temp = r["chi2"] if r["ok"] else DBL_MAX
                scale = (r["scale_l"] + r["scale_p"] if r["ok"] else 0.0) + 1e-3
                rho = (current - temp) / scale
                if rho > 0 and math.isfinite(temp):
                    alpha = min(1.0 - math.pow(2 * rho - 1, 3), 2.0 / 3.0)
                    s["lam"] *= max(1.0 / 3.0, alpha)
                    ni = 2.0
                    current = temp
                else:
                    s["lam"] *= ni
                    ni *= 2
                    s["carry"] |= RESTORE  # pop(): before anything else touches the estimates
                qmax += 1
                res["chi2_final"] = current
                if not (rho < 0 and qmax < 10 and not stop(2 * len(rounds) - 1)):
                    break
            if qmax == 10 or rho == 0:
                return  # Terminate
            n_bad = n_bad + 1 if (ini - current) * 1e3 < ini else 0
            if n_bad >= 3:
                return

    first_optimize = [True]  # chi2_initial is the first optimize()'s
    if c.full_ba:
        optimize(c.its0, c.robust)
    else:
        optimize(c.its0, True)
        first_optimize[0] = False
        if stop(2 * len(rounds)):  # pbStopFlag between the two optimisations
            res["status"] = ABORTED
        else:
            s["carry"] |= CLASS0
            n = len(rounds)
            optimize(c.its1, False)
            if len(rounds) == n:  # no trial carried the classification: a round of its own
                rounds.append((s["carry"], s["lam"]))
                s["carry"] = 0
        s["carry"] |= CLASS1
    if s["carry"]:
        rounds.append((s["carry"], s["lam"]))
    return rounds, res, used[0]


# --------------------------------------------------------------------------------------------- the driver's two calls
def drive(lib, c):
    lib.pol_start(int(c.full_ba), int(c.robust), int(c.vio_local), c.its0, c.its1, c.lambda_init)
    if c.skip is not None:
        lib.pol_skip(c.skip)
    rounds, used, shard_stop = [], 0, False
    fp, lam = (ctypes.c_int * 2)(), ctypes.c_double()
    for r in range(1000):
        stop_now = shard_stop if c.sharded else (c.stop_time is not None and 2 * r >= c.stop_time)
        lib.pol_plan(int(stop_now), 7 if c.sharded else 0, fp, ctypes.byref(lam))
        flags = fp[0]
        assert fp[1] == (7 if c.sharded else 0)
        if not flags:
            break
        rounds.append((flags, lam.value))
        if not flags & TRIAL:
            continue
        t = c.script[used]
        used += 1
        o = (ctypes.c_double * 9)(t["chi0"], t["chi2"], t["scale_l"], t["scale_p"], t["lam"], t["ok"], t["np"], t["chig0"], t["chig"])
        sc = (ctypes.c_double * 4)(*t["sc"]) if t["sc"] is not None else None
        if sc is not None and lib.pol_shard_stop(flags, sc):
            shard_stop = True
        stopped = shard_stop if c.sharded else (c.stop_time is not None and 2 * r + 1 >= c.stop_time)
        lib.pol_digest(flags, o, sc, int(stopped))
        if sc is not None:  # the totals land in the record
            assert (o[0], o[1], o[2]) == (t["sc"][0] + t["chig0"], t["sc"][1] + t["chig"], t["sc"][2])
    else:
        raise AssertionError("the policy never finished")
    ri, rd = (ctypes.c_int * 4)(), (ctypes.c_double * 2)()
    lib.pol_result(ri, rd)
    res = dict(status=ri[0], lm_iterations=ri[1], lm_trials=ri[2], chi2_initial=rd[0], chi2_final=rd[1])
    assert ri[3] == 0
    return rounds, res, used


def falling(n, start=100.0, f=0.5, **kw):
    """n accepted trials, each a large gain"""
    out, chi = [], start
    for _ in range(n):
        chi *= f
        out.append(rec(chi, chi0=start, **kw))
    return out


REJ = dict(chi2=150.0)  # worse than anything a script holds: rho < 0
CASES = {
    "accepted_until_its0_runs_out": Case(falling(5), its0=3, its1=2),
    "rejected_then_accepted": Case([rec(50.0), rec(**REJ), rec(**REJ), rec(20.0), rec(10.0)] + falling(8, 10.0), its0=3, its1=2),
    "ten_rejections": Case([rec(50.0)] + [rec(**REJ)] * 10 + falling(4, 50.0), its0=4, its1=3),
    "ten_rejections_at_begin": Case([rec(**REJ)] * 10 + [rec(60.0), rec(30.0)], its0=4, its1=2),
    "three_small_gains": Case([rec(99.99), rec(99.98), rec(99.97), rec(99.96), rec(50.0), rec(25.0)], its0=6, its1=2),
    "small_gains_interrupted": Case([rec(99.99), rec(99.98), rec(50.0), rec(49.999), rec(49.998), rec(49.997), rec(1.0)], its0=9, its1=1),
    "rho_zero": Case([rec(50.0), rec(50.0), rec(25.0), rec(25.0)], its0=5, its1=5),
    "solve_failed": Case([rec(50.0), rec(10.0, ok=0), rec(40.0), rec(5.0, ok=0), rec(30.0)] + falling(3, 30.0), its0=3, its1=2),
    "no_active_vertex": Case([rec(0.0, np_=0), rec(0.0, np_=0)]),
    "no_active_vertex_second_stage": Case(falling(2) + [rec(0.0, np_=0)], its0=2, its1=4),
    "its0_zero": Case(falling(3), its0=0, its1=3),
    "its1_zero": Case(falling(3), its0=3, its1=0),
    "its1_zero_after_rejection": Case([rec(50.0), rec(**REJ)] * 1 + [rec(**REJ)] * 9, its0=3, its1=0),
    "both_zero": Case([], its0=0, its1=0),
    "stop_mid_trial": Case(falling(4), its0=4, its1=3, stop_time=3),
    "stop_mid_rejected_trial": Case([rec(50.0), rec(**REJ), rec(25.0)], its0=4, its1=3, stop_time=3),
    "stop_in_second_stage": Case(falling(6), its0=2, its1=5, stop_time=7),
    "stop_between_stages": Case(falling(4), its0=2, its1=3, stop_time=4),
    "stop_before_call": Case([], skip=ABORTED),
    "no_free_pose": Case([], skip=NO_FREE_POSE),
    "full_ba_robust": Case(falling(3, lam=2.5e-4) + [rec(**REJ), rec(1.0)], its0=4, full_ba=True, robust=True),
    "full_ba_plain": Case([rec(50.0, lam=7e-2), rec(**REJ), rec(20.0), rec(10.0)], its0=3, full_ba=True),
    "full_ba_ends_rejected": Case([rec(50.0), rec(**REJ), rec(**REJ)] + [rec(**REJ)] * 8, its0=3, full_ba=True),
    "full_ba_no_iterations": Case([], its0=0, full_ba=True),
    "full_ba_stop": Case(falling(5), its0=5, full_ba=True, stop_time=3),
    "vio_lambda_init_prelevel_once": Case(falling(2, lam=123.0) + [rec(**REJ)] + falling(4, 25.0, lam=456.0), its0=2, its1=3,
                                          vio_local=True, lambda_init=1e-1),
    "vio_full_ba_device_lambda": Case(falling(3, lam=3e-3), its0=3, full_ba=True, robust=True, vio_local=False, lambda_init=1e-1),
    "sharded_totals": Case([rec(1e9, chi0=1e9, scale_l=1e9, chig0=30.0, chig=20.0, sc=[70.0, 30.0, 2.0, 0.0]),
                            rec(1e9, scale_l=1e9, chig=40.0, sc=[70.0, 0.0, 3.0, 0.0]),
                            rec(1e9, scale_l=1e9, chig=10.0, sc=[15.0, 0.0, 1.5, 0.0]),
                            rec(1e9, chi0=1e9, scale_l=1e9, chig0=10.0, chig=5.0, sc=[15.0, 0.0, 0.5, 0.0]),
                            rec(1e9, scale_l=1e9, chig=2.0, sc=[3.0, 0.0, 0.25, 0.0])], its0=2, its1=2, vio_local=True,
                           lambda_init=1e-2),
    "sharded_stop_from_fourth_scalar": Case([rec(1e9, chi0=1e9, chig0=30.0, chig=20.0, sc=[70.0, 30.0, 2.0, 0.0]),
                                             rec(1e9, chig=10.0, sc=[25.0, 0.0, 3.0, 2.0]),
                                             rec(1e9, chig=5.0, sc=[10.0, 0.0, 3.0, 2.0])], its0=4, its1=2, vio_local=True,
                                            lambda_init=1e-2),
}


@pytest.mark.parametrize("name", list(CASES))
def test_policy_matches_the_reference_loops(lib, name):
    c = CASES[name]
    want_rounds, want_res, want_used = model(c)
    got_rounds, got_res, got_used = drive(lib, c)
    for r, (g, w) in enumerate(zip(got_rounds, want_rounds)):
        assert g == w, "round %d: control word / lambda %r, the reference loops give %r" % (r, g, w)  # doubles: exact
    assert len(got_rounds) == len(want_rounds)
    assert got_used == want_used
    assert got_res == want_res


def test_scripts_reach_what_they_are_for(lib):
    """The scripts above take the paths their names say (against the restatement alone, so a slip in a script shows)."""
    flags = {n: [f for f, _ in model(c)[0]] for n, c in CASES.items()}
    res = {n: model(c)[1] for n, c in CASES.items()}
    assert res["accepted_until_its0_runs_out"]["lm_iterations"] == 5 and res["accepted_until_its0_runs_out"]["lm_trials"] == 5
    assert any(f & RESTORE for f in flags["rejected_then_accepted"])
    assert res["ten_rejections"]["lm_trials"] >= 11 and res["ten_rejections_at_begin"]["lm_trials"] == 12
    assert res["three_small_gains"]["lm_iterations"] == 3 + 2  # the first optimize() stops after its third small gain
    assert res["small_gains_interrupted"]["lm_iterations"] == 6 + 1
    assert res["rho_zero"]["lm_trials"] == 4
    assert res["no_active_vertex"] == dict(status=OK, lm_iterations=0, lm_trials=0, chi2_initial=0.0, chi2_final=0.0)
    assert flags["both_zero"] == [CLASS0, CLASS1]
    assert res["stop_mid_trial"]["status"] == ABORTED and res["stop_between_stages"]["status"] == ABORTED
    assert res["stop_in_second_stage"]["status"] == OK and res["stop_in_second_stage"]["lm_trials"] == 4
    assert res["stop_before_call"]["status"] == ABORTED and flags["stop_before_call"] == []
    assert all(f & ROBUST for f in flags["full_ba_robust"] if f & TRIAL) and not any(f & ROBUST for f in flags["full_ba_plain"])
    assert flags["full_ba_ends_rejected"][-1] == RESTORE and not any(f & (CLASS0 | CLASS1) for f in flags["full_ba_robust"])
    assert sum(bool(f & PRELEVEL) for f in flags["vio_lambda_init_prelevel_once"]) == 1
    assert model(CASES["vio_lambda_init_prelevel_once"])[0][0][1] == 1e-1 and model(CASES["full_ba_robust"])[0][0][1] == -1.0
    assert res["sharded_totals"]["chi2_initial"] == 100.0 and res["sharded_totals"]["chi2_final"] == 5.0
    assert res["sharded_stop_from_fourth_scalar"]["status"] == ABORTED and res["sharded_stop_from_fourth_scalar"]["lm_trials"] == 2
