"""Loop verification: Optimizer::OptimizeSim3 for a list of visits in one launch (vieo_optimize_sim3) against the
restatement of tests/loop_optimize_ref.py and the golden cases of tests/golden/loop_optimize_golden.npz.

The CPU tests come first and check the restatement itself -- against the truth of a noise-free scene, and every Jacobian
block of both edge modes against central differences through the restated retraction, PINNING the relation it finds per
block (the expressions of the reference's MODE 2 are the specification, not its derivatives) --, then the kernel's lane
functions compiled for the host (tests/emul/sim3_opt_emul.cc) against the restatement on every golden case, then the
paths of the sequence.  The GPU tests ask match12, nBad, nInliers and every accepted / rejected trial exactly, S12 and
the trials' chi2 within 4 x the spread tests/golden/LOOP_OPTIMIZE.md records for the case (the factor: the device order
of operations is one more than the variants sample).

Figures, measured on the host build when this file was written: S12 of the 1-lane and of the 64-lane build differ from
the unperturbed restatement by at most the recorded spread on every case (see LOOP_OPTIMIZE.md)."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import loop_optimize_ref as ref
from tests import loop_verify_ref
from tests import pose_graph_ref as pgr
from tests.golden import make_loop_optimize_golden as gen
from vieo_slam_amd import _lib
from vieo_slam_amd import loop_closing as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(gen.CASES)
TH2 = gen.TH2
LM0 = pgr.Libm(0)


@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "loop_optimize_golden.npz"))


@functools.lru_cache(maxsize=None)
def _case(name):
    """the key frames, the visit and the recorded results of a golden case"""
    Z, p = _golden(), name + "/"
    g = lambda k: Z[p + k]
    return dict(kf1=gen.unpack_kf(Z, p + "kf1/"), kf2=gen.unpack_kf(Z, p + "kf2/"), fix=bool(g("fix")),
                visit=(0, float(g("s12_in")), g("R12_in"), g("t12_in"), g("match_in")),
                want={k: g(k) for k in ("s12", "R12", "t12", "match", "n_inliers", "n_bad", "n_corr", "returned0", "iterations",
                                        "trials", "trace", "erased", "i1", "chi_check", "s12_spread", "chi_spread", "truth",
                                        "outliers")})


@functools.lru_cache(maxsize=None)
def _problem(name):
    c = _case(name)
    return ref.problem(c["kf1"], c["kf2"], c["visit"][4])


def _s12_diff(got, want):
    return max(abs(got[0] - float(want["s12"])), float(np.abs(np.asarray(got[1]) - want["R12"]).max()),
               float(np.abs(np.asarray(got[2]) - want["t12"]).max()))


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the restatement
def test_the_golden_file_is_the_restatement():
    """the stored results are what the restatement gives today on the stored key frames (two cases, unperturbed)"""
    for name in ("p65_o5", "kb840"):
        c = _case(name)
        m, S, n_in, d = ref.optimize_sim3(c["kf1"], c["kf2"], *c["visit"][1:], TH2, c["fix"])
        w = c["want"]
        assert np.array_equal(m, w["match"]) and n_in == w["n_inliers"] and d["n_bad"] == w["n_bad"]
        assert np.array_equal(np.array(d["trace"])[:, 3], w["trace"][:, 3])
        assert _s12_diff(S, w) <= 4 * float(w["s12_spread"])


@pytest.mark.parametrize("fix", [False, True])
def test_restatement_against_the_truth_of_a_noise_free_scene(fix):
    """observations replaced by the exact projections of the points: from a perturbed start chi2 falls, S12 moves towards
    the truth, nothing is erased (the factors are recorded in LOOP_OPTIMIZE.md's table for the noisy cases)"""
    s = lc.make_loop_optimize_scene(7, 60, 0)
    c, s12, R12, t12, m = s["visit"]
    ts, tR, tt = s["truth"]
    if fix:
        s12 = ts  # a fixed scale stays where it starts
    prob, i1, i2 = ref.problem(s["kf1"], s["kf2s"][0], m)
    cam = prob["cams"][0]
    for X, key in ((prob["X1"], "obs1"), (prob["X2"], "obs2")):  # the camera frame IS the rig frame here (Tcr = I)
        prob[key] = ref.project(cam, X, LM0, False)[0]
    d = ref.run(prob, ref.state_from_sim3(R12, t12, s12, LM0), TH2, fix, LM0)
    S = ref.state_to_sim3(d["st"], LM0)
    tr = np.array(d["trace"])
    before = max(abs(s12 - ts), np.abs(R12 - tR).max(), np.abs(t12 - tt).max())
    after = max(abs(S[0] - ts), np.abs(S[1] - tR).max(), np.abs(S[2] - tt).max())
    print("noise-free, fixed scale %d: chi2 %.3e -> %.3e, distance to the truth %.3e -> %.3e" % (fix, tr[0, 0], tr[:, 1].min(), before, after))
    assert d["n_bad"] == 0 and d["n_inliers"] == len(i1) and not d["erased"].any()
    assert tr[tr[:, 3] == 1, 1].min() < 1e-3 * tr[0, 0]
    assert after < 0.1 * before


def _camera_for(rig, with_tcb):
    if rig == "pinhole":
        rec, T = lc.pinhole_camera()[0], np.eye(4)[:3].copy()
        if with_tcb:
            T[:, 3] = [0.1, -0.05, 0.02]
    else:
        from vieo_slam_amd.synth_ba import camera_rig
        cams, _, Tcr = camera_rig(rig, with_tcr=True, n_cams=2)
        rec, T = cams[1], np.array(Tcr[1], np.float64)[:3].copy()
        assert np.abs(T[:, 3]).max() > 0.01
        if not with_tcb:
            T[:, 3] = 0
    return ref.camera(rec, T.reshape(-1))


@pytest.mark.parametrize("s", [0.9, 1.0, 1.1])
@pytest.mark.parametrize("with_tcb", [False, True])
@pytest.mark.parametrize("rig", ["pinhole", "radtan", "kb8"])
def test_jacobian_blocks_against_central_differences(rig, with_tcb, s):
    """Every block of both modes against central differences of Pc through the restated retraction, times the edge's own
    Jproj (so the camera model's Jacobian, which the Radtan model of the reference states approximately, stays out).
    What it finds, and pins:
      MODE 1 (EdgeReprojectPRS): position, rotation and scale blocks are the derivatives.
      MODE 2 (EdgeReprojectPRSInv): the rotation block is the derivative; the position block is s TIMES the derivative (it
      lacks the factor 1 / s of the scaled translation); the scale column is NOT the derivative: with `tcw *= scale` the
      whole of Pc scales with 1 / s, so Jproj dPc/ds = -Jproj Pc / s is zero for every central projection, while the
      column is (J_s + Jproj tcw)(-scale^2) = -(1 - 1 / s) / s^2 Jproj Rcw X, which vanishes only at s = 1."""
    cam = _camera_for(rig, with_tcb)
    R12, t12 = lc.rodrigues(np.array([0.05, -0.03, 0.04])), np.array([0.2, -0.1, 0.15])
    st = ref.state_from_sim3(R12, t12, s, LM0)
    X, obs = np.array([[0.5, -0.3, 6.0]]), np.array([[300., 200.]])
    h = 1e-6
    for mode in (1, 2):
        parts = {}
        e, J = ref.edge(mode, cam, st, X, obs, LM0, True, parts)
        Jproj = parts["Jproj"][0].reshape(2, 3)
        N = np.zeros((2, 7))
        for k in range(7):
            pc = []
            for sign in (1, -1):
                d = [0.0] * 7
                d[k] = sign * h
                pp = {}
                ref.edge(mode, cam, ref.inc_small(st, d, False, LM0), X, obs, LM0, False, pp)
                pc.append(pp["Pc"][0])
            N[:, k] = Jproj @ ((pc[0] - pc[1]) / (2 * h))
        A = J[0]
        scale_of = np.abs(A[:, :6]).max()
        close = lambda a, b: np.abs(a - b).max() < 1e-7 * scale_of
        assert close(A[:, 3:6], N[:, 3:6]), (mode, "rotation")
        if mode == 1:
            assert close(A[:, :3], N[:, :3]) and close(A[:, 6], N[:, 6])
            continue
        assert close(A[:, :3], s * N[:, :3]), "position block = s x derivative"
        assert (s == 1.0) or not close(A[:, :3], N[:, :3])
        assert np.abs(N[:, 6]).max() < 1e-7 * scale_of, "e21 does not depend on the scale"
        Rcw, Xs = np.array(parts["Rcw"]).reshape(3, 3), X[0]
        stated = -(1 - 1 / s) / (s * s) * (Jproj @ (Rcw @ Xs))
        assert np.abs(A[:, 6] - stated).max() < 1e-9 * scale_of
        assert (np.abs(A[:, 6]).max() > 1e-3 * scale_of) == (s != 1.0)


@pytest.mark.parametrize("rig", ["pinhole", "kb8"])
def test_projection_jacobian_of_the_exact_models(rig):
    cam = _camera_for(rig, True)
    P = np.array([[0.4, -0.2, 5.0]])
    ref.ROUND_UV = False
    try:
        _, J = ref.project(cam, P, LM0, True)
        N = np.zeros((2, 3))
        for k in range(3):
            d = np.zeros((1, 3))
            d[0, k] = 1e-6
            N[:, k] = (ref.project(cam, P + d, LM0, False)[0][0] - ref.project(cam, P - d, LM0, False)[0][0]) / 2e-6
    finally:
        ref.ROUND_UV = True
    assert np.abs(J[0].reshape(2, 3) - N).max() < 1e-6 * np.abs(N).max()


def test_i2_is_the_smallest_key_of_a_point_held_by_two_keys():
    c = _case("radtan40")
    kf2 = c["kf2"]
    prob, i1, i2 = _problem("radtan40")
    m = c["visit"][4]
    twice = 0
    for a, b in zip(i1, i2):
        held = np.flatnonzero(kf2.mp_id == kf2.mp_id[m[a]])
        assert b == held.min()
        twice += len(held) > 1 and m[a] != held.min()
    assert twice > 0  # some match12 entry names the larger key: the observation is still the smaller one's
    assert (prob["cam2"][np.flatnonzero(i2 != m[i1])] == kf2.n_cams + kf2.cam_of_key[i2[i2 != m[i1]]]).all()


def test_no_correspondence_returns_zero_and_touches_nothing():
    c = _case("p10")
    _, s12, R12, t12, m = c["visit"]
    empty = np.full_like(m, -1)
    out, S, n_in, d = ref.optimize_sim3(c["kf1"], c["kf2"], s12, R12, t12, empty, TH2)
    assert n_in == 0 and d is None and np.array_equal(out, empty) and S[0] == s12 and np.array_equal(S[1], R12)


def test_sequence_five_more_without_outliers_ten_with(monkeypatch):
    asked = []
    real = ref._Run.optimize

    def spy(self, st, iters):
        asked.append(iters)
        return real(self, st, iters)
    monkeypatch.setattr(ref._Run, "optimize", spy)
    for name, want in (("p64", [5, 5]), ("p64_o5", [5, 10]), ("p13_o4", [5])):
        del asked[:]
        c = _case(name)
        ref.optimize_sim3(c["kf1"], c["kf2"], *c["visit"][1:], TH2, c["fix"])
        assert asked == want, name


@pytest.mark.parametrize("name", ["p13_o4", "p13_o4_fix"])
def test_return_zero_keeps_s12_and_the_first_round_erasures(name):
    c = _case(name)
    _, s12, R12, t12, m = c["visit"]
    out, S, n_in, d = ref.optimize_sim3(c["kf1"], c["kf2"], s12, R12, t12, m, TH2, c["fix"])
    assert n_in == 0 and d["returned0"] == 1 and d["n_correspondences"] - d["n_bad"] < 10
    assert S[0] == s12 and S[1].tobytes() == np.asarray(R12, np.float64).tobytes() and S[2].tobytes() == np.asarray(t12, np.float64).tobytes()
    gone = np.flatnonzero((m >= 0) & (out < 0))
    assert len(gone) == d["n_bad"] >= 4 and set(c["want"]["outliers"].tolist()) <= set(gone.tolist())
    assert (d["erased"] <= 1).all() and not d["chi_check"][1].any()


def test_stale_read_mechanism():
    """after an optimize() whose last trial was rejected, a check reads the chi2 of the REJECTED state (pop() does not
    restore the errors): bit for bit those of a fresh evaluation at the rejected state.  In every case found the rejected
    step is smaller than the float rounding of (u, v) moves, so the kept state's errors are the same bits: that is why the
    search LOOP_OPTIMIZE.md records found no seed where the stale read changes a classification."""
    c = _case("p65")
    prob, i1, i2 = _problem("p65")
    _, s12, R12, t12, m = c["visit"]
    run = ref._Run(prob, TH2, False, LM0, "forward")
    states = []
    real = ref.inc_small
    try:
        ref.inc_small = lambda st, d, fix, lm: states.append(real(st, d, fix, lm)) or states[-1]
        kept, _, _ = run.optimize(ref.state_from_sim3(R12, t12, s12, LM0), 5)
    finally:
        ref.inc_small = real
    assert run.trace[-1][3] == 0.0 and states[-1] != kept
    read = run.chi.copy()
    run.errors(states[-1])
    assert read.tobytes() == run.chi.tobytes()
    assert int(_golden()["stale/found"]) == 0


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the kernel's lane functions compiled for the host
CORR_DTYPE = np.dtype([("X1", "<f8", 3), ("X2", "<f8", 3), ("obs1", "<f8", 2), ("obs2", "<f8", 2), ("info1", "<f8"), ("info2", "<f8"),
                       ("cam1", "<i4"), ("cam2", "<i4"), ("i1", "<i4"), ("i2", "<i4")], align=True)


@functools.lru_cache(maxsize=None)
def _emul():
    out = os.path.join(ROOT, "tests", "emul", "libsim3_opt_emul.so")
    csrc = os.path.join(ROOT, "vieo_slam_amd", "csrc")
    deps = [os.path.join(ROOT, "tests", "emul", "sim3_opt_emul.cc")] + [os.path.join(csrc, f) for f in (
        "sim3_optimize_device.h", "cam_project.h", "sim3_device.h", "lba_policy.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", out, deps[0], "-lm"])
    L = ctypes.CDLL(out)
    L.emul_s3o_edge.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_double] + [ctypes.c_void_p] * 4
    L.emul_s3o_visit.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                 ctypes.c_float, ctypes.c_int] + [ctypes.c_void_p] * 5
    L.emul_s3o_from_sim3.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p]
    L.emul_s3o_to_sim3.argtypes = [ctypes.c_void_p] * 4
    assert L.emul_s3o_corr_size() == CORR_DTYPE.itemsize == 112
    return L


def _emul_visit(name, n_lanes):
    """the whole visit on the host build: (S12, ints, erased, chi_check, trace)"""
    L, c = _emul(), _case(name)
    prob, i1, i2 = _problem(name)
    n = len(i1)
    corr = np.zeros(n, CORR_DTYPE)
    for k in ("X1", "X2", "obs1", "obs2", "info1", "info2", "cam1", "cam2"):
        corr[k] = prob[k]
    corr["i1"], corr["i2"] = i1, i2
    cams = np.concatenate([ref.cam_flat(cm) for cm in prob["cams"]])
    _, s12, R12, t12, m = c["visit"]
    st_in, st_out = np.zeros(8), np.zeros(8)
    R12c, t12c = np.ascontiguousarray(R12, np.float64).reshape(-1), np.ascontiguousarray(t12, np.float64)
    L.emul_s3o_from_sim3(R12c.ctypes.data, t12c.ctypes.data, float(s12), st_in.ctypes.data)
    ints, erased = np.zeros(8, np.int32), np.zeros(max(n, 1), np.int32)
    chi_check, trace = np.zeros((2, n, 2)), np.zeros((lc.SIM3_OPT_MAX_TRIALS, 4))
    L.emul_s3o_visit(n_lanes, n, corr.ctypes.data, len(prob["cams"]), cams.ctypes.data, st_in.ctypes.data, TH2, int(c["fix"]),
                     st_out.ctypes.data, ints.ctypes.data, erased.ctypes.data, chi_check.ctypes.data, trace.ctypes.data)
    Ro, to, so = np.zeros(9), np.zeros(3), ctypes.c_double(0)
    L.emul_s3o_to_sim3(st_out.ctypes.data, Ro.ctypes.data, to.ctypes.data, ctypes.byref(so))
    same_state = st_in.tobytes() == st_out.tobytes()
    return (so.value, Ro.reshape(3, 3), to), ints, erased[:n], chi_check, trace[:ints[3]], same_state


def _check_against_golden(name, S, n_inliers, n_bad, erased, trace, iterations, trials, returned0, what):
    w = c = _case(name)["want"]
    tol_s, tol_chi = 4 * float(w["s12_spread"]), 4 * w["chi_spread"]
    d_s = 0.0 if returned0 else _s12_diff(S, w)
    d_chi = np.abs(trace[:, :2] - w["trace"][:, :2]) if trace.shape == w["trace"].shape else None
    print("%s %s: |S12 - restated| %.2e (recorded spread %.2e), worst chi2 difference / its spread %s" % (
        what, name, d_s, float(w["s12_spread"]),
        "n/a" if d_chi is None else "%.2f" % float((d_chi / np.maximum(w["chi_spread"], 1e-300)).max())))
    assert n_inliers == int(w["n_inliers"]) and n_bad == int(w["n_bad"]) and int(returned0) == int(w["returned0"])
    assert np.array_equal(erased, c["erased"])
    assert trace.shape == w["trace"].shape and np.array_equal(trace[:, 3], w["trace"][:, 3])
    assert list(iterations) == w["iterations"].tolist() and list(trials) == w["trials"].tolist()
    assert d_s <= tol_s
    assert (d_chi <= tol_chi).all()


@pytest.mark.parametrize("name", ["p65_o5", "radtan40", "kb840"])
def test_host_build_edges_equal_the_restatement(name):
    L = _emul()
    prob, i1, i2 = _problem(name)
    c = _case(name)
    _, s12, R12, t12, m = c["visit"]
    st = ref.state_from_sim3(R12, t12, s12, LM0)
    q, p = np.array(st[1]), np.array(st[0])
    worst = 0.0
    for mode, X, obs, cam in ((1, prob["X2"], prob["obs1"], prob["cam1"]), (2, prob["X1"], prob["obs2"], prob["cam2"])):
        for k in range(len(i1)):
            cm = prob["cams"][int(cam[k])]
            e_ref, J_ref = ref.edge(mode, cm, st, X[k:k + 1], obs[k:k + 1], LM0, True)
            e, J = np.zeros(2), np.zeros(14)
            flat, Xk, ok = ref.cam_flat(cm), np.ascontiguousarray(X[k]), np.ascontiguousarray(obs[k])
            L.emul_s3o_edge(mode, flat.ctypes.data, q.ctypes.data, p.ctypes.data, float(st[2]), Xk.ctypes.data, ok.ctypes.data,
                            e.ctypes.data, J.ctypes.data)
            assert np.array_equal(e, e_ref[0]) or np.abs(e - e_ref[0]).max() < 1e-4  # (one float ulp of u, v at most)
            worst = max(worst, np.abs(J.reshape(2, 7) - J_ref[0]).max() / np.abs(J_ref[0]).max())
    assert worst < 1e-12


@pytest.mark.parametrize("n_lanes", [1, 64])
@pytest.mark.parametrize("name", CASES)
def test_host_build_equals_the_restatement(name, n_lanes):
    S, ints, erased, chi_check, trace, same_state = _emul_visit(name, n_lanes)
    _check_against_golden(name, S, ints[0], ints[1], erased, trace, ints[4:6], ints[6:8], ints[2], "host build, %d lanes" % n_lanes)
    w = _case(name)["want"]
    read = w["chi_check"] > 0
    assert np.array_equal(chi_check > 0, read)
    assert np.array_equal(chi_check > TH2, w["chi_check"] > TH2)
    if ints[2]:
        assert same_state and (erased <= 1).all()  # `return 0`: the state is the input bit for bit


# ---------------------------------------------------------------------------------------------------------------------
# GPU
def _device(name, **kw):
    c = _case(name)
    rc, out = lc.optimize_sim3_call(c["kf1"], [c["kf2"]], [c["visit"]], TH2, c["fix"], **kw)
    assert rc == _lib.VIEO_OK, _lib.lib().vieo_last_error()
    return out[0], lc.optimize_sim3_trace(0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_optimize_sim3_equals_the_restatement(name):
    c = _case(name)
    w = c["want"]
    o, t = _device(name)
    erased = np.zeros(int(w["n_corr"]), np.int32)
    assert o["n_correspondences"] == int(w["n_corr"]) and np.array_equal(t["i1"], w["i1"])
    assert np.array_equal(o["match12"], w["match"])
    first = t["chi2"][0]
    bad1 = (first[:, 0] > TH2) | (first[:, 1] > TH2)
    erased[bad1] = 1
    second = t["chi2"][1]
    erased[(second[:, 0] > TH2) | (second[:, 1] > TH2)] = 2
    returned0 = o["n_inliers"] == 0 and o["n_correspondences"] - o["n_bad"] < 10
    _check_against_golden(name, (o["s12"], o["R12"], o["t12"]), o["n_inliers"], o["n_bad"], erased, t["trials"], o["iterations"],
                          o["trials"], returned0, "device")
    if returned0:
        _, s12, R12, t12, m = c["visit"]
        assert o["s12"] == s12 and o["R12"].tobytes() == np.asarray(R12, np.float64).tobytes() and o["t12"].tobytes() == np.asarray(t12, np.float64).tobytes()
    rel = np.abs(t["chi2"] - w["chi_check"]) / np.maximum(w["chi_check"], 1e-300)
    assert np.array_equal(t["chi2"] > 0, w["chi_check"] > 0) and rel[w["chi_check"] > 0].max() < 1e-9


def _batch_visits():
    """6 visits of one call over 2 candidates (the same key frame in two slots): two name candidate 0 with different S12,
    one is a return-0 case (13 correspondences, 5 of them the planted outliers), visits 1 and 4 differ only in the slot"""
    A, B = _case("p65_o5"), _case("p65")
    assert A["kf1"].keys.tobytes() == B["kf1"].keys.tobytes() and A["kf2"].keys.tobytes() == B["kf2"].keys.tobytes()
    a, b = A["visit"], B["visit"]
    turned = (a[1] * 1.004, lc.rodrigues(np.array([0.001, 0.002, -0.001])) @ a[2], a[3] + 0.01)
    few = a[4].copy()
    few[np.flatnonzero(few >= 0)[13:]] = -1
    visits = [(0,) + a[1:], (1,) + b[1:], (0,) + turned + (a[4],), (1,) + a[1:4] + (few,), (0,) + b[1:], (1,) + turned + (b[4],)]
    return A["kf1"], [A["kf2"], B["kf2"]], visits


def _bytes_of(o, t):
    return b"".join([o["match12"].tobytes(), np.float64(o["s12"]).tobytes(), o["R12"].tobytes(), o["t12"].tobytes(),
                     np.array([o["n_inliers"], o["n_bad"], o["n_correspondences"]] + o["iterations"] + o["trials"], np.int32).tobytes(),
                     t["trials"].tobytes(), t["chi2"].tobytes()])


@pytest.mark.gpu
def test_optimize_sim3_batch_equals_single_visits_and_itself():
    kf1, kf2s, visits = _batch_visits()
    runs = []
    for _ in range(2):
        rc, out = lc.optimize_sim3_call(kf1, kf2s, visits, TH2, False)
        assert rc == _lib.VIEO_OK
        runs.append([_bytes_of(o, lc.optimize_sim3_trace(v)) for v, o in enumerate(out)])
        results = out
    assert runs[0] == runs[1]
    for v, visit in enumerate(visits):
        rc, out = lc.optimize_sim3_call(kf1, kf2s, [visit], TH2, False)
        assert rc == _lib.VIEO_OK and _bytes_of(out[0], lc.optimize_sim3_trace(0)) == runs[0][v], v
    assert runs[0][0] != runs[0][2] and runs[0][1] == runs[0][4]
    assert results[3]["n_inliers"] == 0 and results[3]["n_bad"] >= 4 and results[3]["n_correspondences"] == 13
    assert results[0]["n_inliers"] == int(_case("p65_o5")["want"]["n_inliers"])


@pytest.mark.gpu
def test_search_by_sim3_then_optimize_sim3_equals_the_restatements_chained():
    s = lc.make_loop_pair_scene(12, n_cands=2)
    kf1, kf2s = s["kf1"], s["kf2s"]
    entry = np.full(len(kf1.keys), -1, np.int32)
    for i1, i2 in sorted(s["pairs"][0].items())[2::6]:
        entry[i1] = i2
    s12, R12, t12 = s["sim3"][0]
    (m_dev, n_found), = lc.SearchBySim3(kf1, kf2s, [(0, s12, R12, t12, entry)])
    m_ref, n_ref = loop_verify_ref.search_by_sim3(kf1, kf2s[0], s12, R12, t12, entry)[:2]
    assert np.array_equal(m_dev, m_ref) and n_found == n_ref > 40
    visit = (0, float(s12), np.asarray(R12, np.float64), np.asarray(t12, np.float64), m_dev)
    scene = dict(kf1=kf1, kf2s=kf2s, visit=visit)
    base, sp = gen.examine(scene, False)
    assert base is not None, sp
    m, S, n_in, d = base
    (got_m, got_S, got_n), = lc.OptimizeSim3(kf1, kf2s, [visit], TH2, False)
    assert np.array_equal(got_m, m) and got_n == n_in > 20
    diff = max(abs(got_S[0] - S[0]), np.abs(got_S[1] - S[1]).max(), np.abs(got_S[2] - S[2]).max())
    print("composition: |S12 - restated| %.2e, spread %.2e" % (diff, sp["s12"]))
    assert diff <= 4 * sp["s12"]


@pytest.mark.gpu
def test_optimize_sim3_invalid_arguments_touch_nothing():
    c = _case("p64_o5")
    kf1, kf2 = c["kf1"], c["kf2"]
    _, s12, R12, t12, m = c["visit"]
    _device("p64_o5")  # a valid call: its trace must survive the refused ones
    tap = lc.optimize_sim3_trace(0)

    def refused(kf1_, kf2s_, visits, th2=TH2):
        before = [(np.array(v[4], np.int32), float(v[1]), np.array(v[2], np.float64), np.array(v[3], np.float64)) for v in visits]
        rc, out = lc.optimize_sim3_call(kf1_, kf2s_, visits, th2, False)
        assert rc == _lib.VIEO_E_INVALID
        for o, (bm, bs, bR, bt) in zip(out, before):
            assert o["match12"].tobytes() == bm.tobytes() and o["R12"].tobytes() == bR.tobytes() and o["t12"].tobytes() == bt.tobytes()
            assert (o["s12"] == bs or (np.isnan(bs) and np.isnan(o["s12"]))) and o["n_inliers"] == 0 and o["n_correspondences"] == 0
            assert o["iterations"] == [0, 0] and o["trials"] == [0, 0] and o["n_bad"] == 0
        now = lc.optimize_sim3_trace(0)
        assert now["trials"].tobytes() == tap["trials"].tobytes() and now["chi2"].tobytes() == tap["chi2"].tobytes()

    ok = (0, s12, R12, t12, m)
    bad = m.copy()
    bad[5] = len(kf2.keys)
    refused(kf1, [kf2], [ok, (0, s12, R12, t12, bad)])          # a match12 entry outside the candidate's keys
    refused(kf1, [kf2], [(1, s12, R12, t12, m)])                # a candidate outside the table
    refused(kf1, [kf2], [(0, 0.0, R12, t12, m)])                # no scale
    refused(kf1, [kf2], [(0, -1.0, R12, t12, m)])
    refused(kf1, [kf2], [(0, float("nan"), R12, t12, m)])
    refused(kf1, [kf2], [(0, float("inf"), R12, t12, m)])
    Rn = np.array(R12, np.float64)
    Rn[1, 1] = np.nan
    refused(kf1, [kf2], [(0, s12, Rn, t12, m)])
    refused(kf1, [kf2], [ok], th2=0.0)
    refused(kf1, [kf2], [ok], th2=-1.0)

    def broken(field, value, index=None):
        k = lc.LoopKeyFrame(kf2.bow, kf2.points, np.eye(4), kf2.cam_of_key)
        k.rec[:] = kf2.rec
        if index is None:
            k.rec[field] = value
        else:
            k.rec[field][0][index] = value
        return k
    refused(kf1, [kf2, broken("n_levels", 17)], [ok])
    refused(kf1, [kf2, broken("n_cams", 2)], [ok])
    refused(kf1, [kf2, broken("points", 0)], [ok])
    refused(kf1, [kf2, broken("bounds", 100.0, (0, 1))], [ok])
    cam = kf2.cams.copy()
    cam[0]["model"] = 7
    refused(kf1, [kf2, broken("cams", cam.ctypes.data)], [ok])
    octave = lc.LoopKeyFrame(lc.BowKeys(kf2.keys.copy(), kf2.desc, [], kf2.mp_id), kf2.points, np.eye(4))
    octave.keys["octave"][3] = 8
    refused(kf1, [kf2, octave], [ok])
    of_cam = lc.LoopKeyFrame(kf2.bow, kf2.points, np.eye(4), np.full(len(kf2.keys), 1, np.int32))
    refused(kf1, [kf2, of_cam], [ok])


@pytest.mark.gpu
def test_optimize_sim3_without_a_correspondence():
    c = _case("p10")
    _, s12, R12, t12, m = c["visit"]
    empty = np.full_like(m, -1)
    rc, out = lc.optimize_sim3_call(c["kf1"], [c["kf2"]], [(0, s12, R12, t12, empty), c["visit"]], TH2, False)
    assert rc == _lib.VIEO_OK
    o = out[0]
    assert o["n_inliers"] == 0 and o["n_correspondences"] == 0 and np.array_equal(o["match12"], empty)
    assert o["s12"] == s12 and o["R12"].tobytes() == np.asarray(R12, np.float64).tobytes() and o["t12"].tobytes() == np.asarray(t12, np.float64).tobytes()
    assert out[1]["n_inliers"] == int(c["want"]["n_inliers"])
