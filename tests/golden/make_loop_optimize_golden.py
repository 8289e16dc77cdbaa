"""Writes tests/golden/loop_optimize_golden.npz and tests/golden/LOOP_OPTIMIZE.md: the key frames and the visit of every
OptimizeSim3 case of tests/test_loop_optimize.py, the outputs and the trial trace of the unperturbed restatement
(tests/loop_optimize_ref.py, Libm(0), edge order) and the measured spread of N_VARIANTS variants per case -- each a
one-ulp libm (Libm(k)) AND another order of summing the edges (reversed, permuted, 64 strided partial sums then a tree,
which is what the kernel does) --, which the host-build and the device tests take their tolerances from.

    python -m tests.golden.make_loop_optimize_golden

A case is refused (the next seed is taken, here, not a looser test) when the S12 spread exceeds 1e-6, when the variants
disagree on an erased correspondence, on a count or on an accepted trial, or when any chi2_12 / chi2_21 read at either
check lies within a relative 1e-6 of th2 in any variant."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import loop_optimize_ref as R  # noqa: E402
from tests import pose_graph_ref as pgr  # noqa: E402
from vieo_slam_amd import loop_closing as lc  # noqa: E402
from vieo_slam_amd.ba_types import CAMERA_DTYPE  # noqa: E402
from vieo_slam_amd.map_point import FUSE_POINT_DTYPE  # noqa: E402

TH2 = 10.0
SPREAD_BAR = 1e-6
MARGIN = 1e-6
ORDERS = ["reversed", ("perm", 1), "lanes64", ("perm", 2)] * 4
N_VARIANTS = len(ORDERS)  # variant k: Libm(k + 1) with ORDERS[k]
MAX_SEEDS = 40

# name: (pairs, planted outliers, cameras, rig, fixed scale, what the case is there for)
CASES = {}
for _fix in (0, 1):
    _s = "_fix" if _fix else ""
    CASES["p10" + _s] = (10, 0, 1, None, _fix, "inliers")      # the least that does not return 0
    CASES["p13_o4" + _s] = (13, 4, 1, None, _fix, "return0")   # 13 - 4 < 10
    for _n in (64, 65, 130):                                   # one lane each; one lane with two; three strides, ragged
        CASES["p%d%s" % (_n, _s)] = (_n, 0, 1, None, _fix, "inliers")
        CASES["p%d_o5%s" % (_n, _s)] = (_n, 5, 1, None, _fix, "outliers")
CASES["radtan40"] = (40, 0, 2, "radtan", 0, "inliers")
CASES["kb840"] = (40, 0, 2, "kb8", 0, "inliers")
CASES["radtan40_o5_fix"] = (40, 5, 2, "radtan", 1, "outliers")
CASES["kb840_o5"] = (40, 5, 2, "kb8", 0, "outliers")


def pack_kf(kf):
    return dict(x=kf.keys["x"].astype(np.float32), y=kf.keys["y"].astype(np.float32), octave=kf.keys["octave"].astype(np.int32),
                mp_id=kf.mp_id.astype(np.int32), cam=kf.cam_of_key.astype(np.int32), Xw=kf.points["Xw"].astype(np.float32),
                Rcw=kf.Rcw.astype(np.float32), tcw=kf.tcw.astype(np.float32), cams=np.frombuffer(kf.cams.tobytes(), np.uint8),
                Tcr=kf.Tcr.astype(np.float32), bounds=kf.bounds.astype(np.float32), use_distort=np.int32(kf.use_distort))


def unpack_kf(Z, prefix):
    """a LoopKeyFrame from what pack_kf stored (descriptors, normals and distances are not read by OptimizeSim3: zeros)"""
    from vieo_slam_amd.orb_extractor import KEYPOINT_DTYPE
    g = lambda name: Z[prefix + name]
    n = len(g("x"))
    keys = np.zeros(n, KEYPOINT_DTYPE)
    keys["x"], keys["y"], keys["octave"], keys["size"] = g("x"), g("y"), g("octave"), 31.0
    pts = np.zeros(n, FUSE_POINT_DTYPE)
    pts["Xw"] = g("Xw")
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = g("Rcw").reshape(3, 3), g("tcw")
    cams = np.frombuffer(g("cams").tobytes(), CAMERA_DTYPE).copy()
    Tcr = []
    for t in g("Tcr"):
        M = np.eye(4)
        M[:3, :] = t.reshape(3, 4)
        Tcr.append(M)
    b = g("bounds")
    bow = lc.BowKeys(keys, np.zeros((n, 32), np.uint8), [], g("mp_id").copy())
    return lc.LoopKeyFrame(bow, pts, T, g("cam").copy(), cams, Tcr, (float(b[0, 1]), float(b[0, 3])), use_distort=int(g("use_distort")))


def run_case(scene, fix, lm, order):
    c, s12, R12, t12, m = scene["visit"]
    return R.optimize_sim3(scene["kf1"], scene["kf2s"][0], s12, R12, t12, m, TH2, bool(fix), lm, order)


def s12_diff(a, b):
    return max(abs(a[0] - b[0]), float(np.abs(a[1] - b[1]).max()), float(np.abs(a[2] - b[2]).max()))


def examine(scene, fix):
    """(unperturbed result, spreads) or (None, the reason the case is refused)"""
    base = run_case(scene, fix, pgr.Libm(0), "forward")
    m0, S0, n0, d0 = base
    tr0 = np.array(d0["trace"])
    s_spread, chi_spread = 0.0, np.zeros((len(tr0), 2))
    runs = [base] + [run_case(scene, fix, pgr.Libm(k + 1), ORDERS[k]) for k in range(N_VARIANTS)]
    for m, S, n, d in runs:
        read = d["chi_check"][d["chi_check"] > 0]
        if len(read) and (np.abs(read - TH2) < MARGIN * TH2).any():
            return None, "a chi2 within 1e-6 of th2"
        tr = np.array(d["trace"])
        if not np.array_equal(m, m0) or n != n0 or d["n_bad"] != d0["n_bad"] or not np.array_equal(d["erased"], d0["erased"]):
            return None, "the variants disagree on an erased correspondence"
        if tr.shape != tr0.shape or not np.array_equal(tr[:, 3], tr0[:, 3]) or d["iterations"] != d0["iterations"]:
            return None, "the variants disagree on an accepted trial"
        s_spread = max(s_spread, s12_diff(S, S0))
        chi_spread = np.maximum(chi_spread, np.abs(tr[:, :2] - tr0[:, :2]))
    if s_spread > SPREAD_BAR:
        return None, "S12 spread %.1e" % s_spread
    return base, dict(s12=s_spread, chi=chi_spread)


def expectation_met(kind, scene, d, n_in):
    if kind == "return0":
        return d["returned0"] == 1 and d["n_bad"] > 0
    if kind == "inliers":
        return d["returned0"] == 0 and d["n_bad"] == 0 and n_in == d["n_correspondences"]
    planted = set(scene["outliers"])
    return d["returned0"] == 0 and planted <= set(d["i1"][d["erased"] > 0].tolist())


def truth_distance(S, truth):
    return max(abs(S[0] - truth[0]), float(np.abs(np.asarray(S[1]) - truth[1]).max()), float(np.abs(np.asarray(S[2]) - truth[2]).max()))


def find_stale(max_seeds=60):
    """a case whose last trial of the first optimize() is rejected and whose first check differs from a fresh
    re-evaluation of the state the optimisation kept: (seed, pairs, outliers) or None, and what was searched"""
    searched = 0
    for n_pairs, n_out in ((40, 6), (30, 8), (64, 10)):
        for seed in range(max_seeds):
            searched += 1
            scene = lc.make_loop_optimize_scene(1000 + seed, n_pairs, n_out, perturb=3.0)
            got = stale_difference(scene)
            if got is not None and got > 0:
                return (1000 + seed, n_pairs, n_out), searched
    return None, searched


def stale_difference(scene, fix=False):
    """None: the last trial of the first optimize() was accepted; else the number of correspondences whose first-check
    classification differs between the stale read and the errors of the kept state"""
    c, s12, R12, t12, m = scene["visit"]
    lm = pgr.Libm(0)
    prob, i1, i2 = R.problem(scene["kf1"], scene["kf2s"][0], m)
    run = R._Run(prob, TH2, fix, lm, "forward")
    st, it0, tr0 = run.optimize(R.state_from_sim3(R12, t12, s12, lm), 5)
    if run.trace[-1][3] == 1.0:
        return None
    stale = (run.chi[:, 0] > run.th2) | (run.chi[:, 1] > run.th2)
    run.errors(st)
    fresh = (run.chi[:, 0] > run.th2) | (run.chi[:, 1] > run.th2)
    return int((stale != fresh).sum())


def main():
    out, rows, notes = {}, [], []
    for name, (n_pairs, n_out, n_cams, rig, fix, kind) in CASES.items():
        chosen = None
        for seed in range(MAX_SEEDS):
            scene = lc.make_loop_optimize_scene(100 + seed, n_pairs, n_out, n_cams, rig or "radtan")
            base, sp = examine(scene, fix)
            if base is None:
                notes.append("`%s`: seed %d refused (%s)." % (name, 100 + seed, sp))
                continue
            m, S, n_in, d = base
            if not expectation_met(kind, scene, d, n_in):
                notes.append("`%s`: seed %d is not a `%s` case (nBad %d, nInliers %d, returned 0: %d)."
                             % (name, 100 + seed, kind, d["n_bad"], n_in, d["returned0"]))
                continue
            chosen = (100 + seed, scene, base, sp)
            break
        assert chosen, "no seed gives case " + name
        seed, scene, (m, S, n_in, d), sp = chosen
        c, s12, R12, t12, m_in = scene["visit"]
        p = name + "/"
        for k, v in pack_kf(scene["kf1"]).items():
            out[p + "kf1/" + k] = v
        for k, v in pack_kf(scene["kf2s"][0]).items():
            out[p + "kf2/" + k] = v
        tr = np.array(d["trace"])
        out.update({p + "s12_in": np.float64(s12), p + "R12_in": np.asarray(R12, np.float64), p + "t12_in": np.asarray(t12, np.float64),
                    p + "match_in": m_in, p + "fix": np.int32(fix), p + "truth": np.concatenate([[scene["truth"][0]], scene["truth"][1].reshape(-1), scene["truth"][2]]),
                    p + "outliers": np.array(scene["outliers"], np.int32),
                    p + "s12": np.float64(S[0]), p + "R12": np.asarray(S[1]), p + "t12": np.asarray(S[2]), p + "match": m,
                    p + "n_inliers": np.int32(n_in), p + "n_bad": np.int32(d["n_bad"]), p + "n_corr": np.int32(d["n_correspondences"]),
                    p + "returned0": np.int32(d["returned0"]), p + "iterations": np.array(d["iterations"], np.int32),
                    p + "trials": np.array(d["trials"], np.int32), p + "trace": tr, p + "erased": d["erased"], p + "i1": d["i1"].astype(np.int32),
                    p + "chi_check": d["chi_check"], p + "s12_spread": np.float64(sp["s12"]), p + "chi_spread": sp["chi"]})
        start_d, end_d = truth_distance((s12, R12, t12), scene["truth"]), truth_distance(S, scene["truth"])
        rows.append("| %s | %d | %d | %d | %s | %s | %d | %d | %d | %d | %s / %s | %d | %.4e -> %.4e | %.2e -> %.2e | %.1e | %.1e |"
                    % (name, seed, n_pairs, n_out, rig or "pinhole", "fixed" if fix else "free", d["n_correspondences"], d["n_bad"], n_in,
                       d["returned0"], d["iterations"], d["trials"], int((tr[:, 3] == 0).sum()), tr[0, 0], tr[-1, 1] if tr[-1, 3] else tr[-1, 0],
                       start_d, end_d, sp["s12"], float(sp["chi"].max())))
    stale, searched = find_stale()
    out["stale/found"] = np.int32(stale is not None)
    out["stale/case"] = np.array(stale if stale else (0, 0, 0), np.int32)
    np.savez_compressed(os.path.join(HERE, "loop_optimize_golden.npz"), **out)
    with open(os.path.join(HERE, "LOOP_OPTIMIZE.md"), "w") as f:
        f.write("# OptimizeSim3 golden cases: what the restatement's own error is\n\n")
        f.write("Written by `tests/golden/make_loop_optimize_golden.py` together with `loop_optimize_golden.npz`; the host-build and\n"
                "the device tests of `tests/test_loop_optimize.py` take their tolerances from the numbers below.\n\n")
        f.write("The restatement is `tests/loop_optimize_ref.py` (numpy, float64). Each case was run unperturbed (`Libm(0)`, the edges\n"
                "summed in edge order) and in %d variants: variant k uses `Libm(k)` (sin, cos, sqrt, atan2, pow moved by at most one\n"
                "ulp) and another order of summing the edges' contributions to H, b and chi2 (%s; `lanes64` = 64 strided partial sums,\n"
                "then an adjacent-pair tree, which is the kernel's order). \"S12 spread\" is the largest difference between a variant and\n"
                "the unperturbed run over s12, the entries of R12 and of t12; \"chi2 spread\" the largest absolute difference of a trial's\n"
                "chi2 before / after (stored per trial). All variants of a stored case agree on every accepted / rejected trial, on the\n"
                "iteration counts, on every erased correspondence and on the counts, and no chi2 read at a check lies within a relative\n"
                "1e-6 of th2 = %g; a seed that does not is refused (listed below) and the next one taken. \"truth\" is the distance of S12\n"
                "to the scene's true Sim3 (same norm) at entry and at exit: achieved, not asserted as a constant.\n\n"
                % (N_VARIANTS, ", ".join(str(o) for o in ORDERS), TH2))
        f.write("| case | seed | pairs | planted | cameras | scale | nCorr | nBad | nInliers | returned 0 | iterations / trials | rejected trials | chi2 first -> last | truth at entry -> exit | S12 spread | chi2 spread |\n")
        f.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        f.write("\n".join(rows) + "\n\n")
        f.write("Refused or unsuitable seeds:\n\n" + ("\n".join("- " + n for n in notes) if notes else "- none") + "\n\n")
        if stale:
            f.write("The stale read: scene seed %d with %d pairs and %d planted outliers (perturbation x 3) ends its first optimize() on a\n"
                    "rejected trial and classifies differently at the first check than a fresh evaluation of the kept state would\n"
                    "(found after %d scenes); `test_stale_read` pins it.\n" % (stale + (searched,)))
        else:
            f.write("The stale read: %d scenes were searched (40 pairs / 6 outliers, 30 / 8, 64 / 10, 60 seeds each from 1000, start\n"
                    "perturbed x 3) for one whose first optimize() ends on a rejected trial AND whose first check then classifies a\n"
                    "correspondence differently than a fresh evaluation of the kept state; none was found. A rejected last trial is\n"
                    "common (the table's rejected-trial column), but it happens at the noise floor of Project's float rounding: the\n"
                    "rejected step moves no (u, v) by a float ulp, so the stale errors are the kept state's bit for bit.  Starts perturbed\n"
                    "x 20 / 40 / 80 (8 seeds each) never ended an optimize() on a rejected trial.  The mechanism is pinned instead:\n"
                    "`test_stale_read_mechanism` checks that the chi2 a check reads are those of the rejected state bit for bit.\n" % searched)
    print("wrote %d cases; stale:" % len(CASES), stale, "after", searched)


if __name__ == "__main__":
    main()
