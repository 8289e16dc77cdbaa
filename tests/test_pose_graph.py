"""vieo_optimize_essential_graph on the device against tests/golden/pose_graph_golden.npz: the outputs and the trial
trace of the CPU reference (tests/pose_graph_ref.py), with tolerances taken from the reference's own measured spread
under a perturbed libm (tests/golden/POSE_GRAPH.md):

  poses        1e-4 on SE(3) (translation of R | t / s, quaternion), the project's bar; every case's reference spread is
               <= 1e-5; points 1e-4 m
  trace        the leading trials only (before the first with a relative chi2 change below 1e-6 in the reference):
               `accepted` equal, chi2_after within 10 x the recorded spread of that trial
  chi2_final   <= the reference's * (1 + 10 x its recorded relative spread)
  counts       1 <= iterations <= n_iterations, trials <= 10 iterations (never compared with the reference: past the
               leading trials accept / reject is rounding noise)
  linearize    e to 1e-12 absolute, Jacobians edge by edge to 4 x the recorded spread of that edge
  map points   alone (n_iterations = 0): 1e-12 relative to |Pw| before the cast to float"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import pose_graph_ref as R
from vieo_slam_amd import _lib
from vieo_slam_amd import pose_graph as pg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pose_graph_golden.npz")
POSE_BAR = 1e-4
N_ITERATIONS = 20


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


def sims(a):
    a = np.asarray(a, np.float64).reshape(-1, 8)
    return pg.sim3_array(a[:, :4], a[:, 4:7], a[:, 7])


def inputs(name):
    g = golden()
    return dict(Scw=sims(g[name + "/Scw"]), Scw_prior=sims(g[name + "/Scw_prior"]), valid=g[name + "/valid"],
                fixed_kf=int(g[name + "/fixed_kf"]), edge_i=g[name + "/edge_i"], edge_j=g[name + "/edge_j"],
                edge_kind=g[name + "/edge_kind"], edge_info=g[name + "/edge_info"], fix_scale=bool(g[name + "/fix_scale"]))


@functools.lru_cache(maxsize=None)
def device_run(name):
    g = golden()
    return pg.optimize_essential_graph(**inputs(name), n_iterations=N_ITERATIONS, lambda_init=float(g[name + "/lambda_init"]))


def pose_errors(name, out):
    g = golden()
    ref = sims(g[name + "/est"])
    valid = g[name + "/valid"]
    worst = 0.0
    for k in range(len(ref)):
        if valid[k]:
            worst = max(worst, *R.pose_distance(R.from_record(ref[k]), R.from_record(out["Scw_opt"][k])))
    return worst


def check_against_golden(name):
    g = golden()
    out = device_run(name)
    lead = int(g[name + "/n_leading"])
    ref_trace, spread = g[name + "/trace"], g[name + "/chi_spread"]
    err = pose_errors(name, out)
    print("%s: pose error %.3e (bar %.0e, reference spread %.1e); %d iterations / %d trials (reference %d / %d); chi2 %.12e -> "
          "%.12e (reference %.12e)" % (name, err, POSE_BAR, float(g[name + "/pose_spread"]), out["lm_iterations"],
                                       out["lm_trials"], int(g[name + "/lm_iterations"]), int(g[name + "/lm_trials"]),
                                       out["chi2_initial"], out["chi2_final"], float(g[name + "/chi2_final"])))
    for k in range(min(lead, len(out["trace"]))):
        print("  trial %d: accepted %d (ref %d)  chi2_after %.15e  |diff| %.2e  spread %.2e" % (
            k, out["trace"]["accepted"][k], int(ref_trace[k, 3]), out["trace"]["chi2_after"][k],
            abs(out["trace"]["chi2_after"][k] - ref_trace[k, 1]), spread[k]))
    assert out["status"] == 0 and out["n_unknowns"] == int(g[name + "/n_unknowns"])
    assert err < POSE_BAR
    assert len(out["trace"]) >= lead >= 2
    for k in range(lead):
        assert int(out["trace"]["accepted"][k]) == int(ref_trace[k, 3]), k
        assert abs(out["trace"]["chi2_after"][k] - ref_trace[k, 1]) <= 10 * spread[k], k
        assert out["trace"]["lambda"][k] == pytest.approx(ref_trace[k, 2], rel=1e-6)
    assert 1 <= out["lm_iterations"] <= N_ITERATIONS and out["lm_trials"] <= 10 * out["lm_iterations"]
    assert out["chi2_final"] <= float(g[name + "/chi2_final"]) * (1 + 10 * float(g[name + "/final_rel_spread"]))
    # Tcw is R | t / s of Scw_opt
    for k in np.flatnonzero(g[name + "/valid"]):
        S = R.from_record(out["Scw_opt"][k])
        assert np.abs(out["Tcw"][k, :, :3] - np.array(R.quat_to_mat(S[0])).reshape(3, 3)).max() < 1e-15
        assert np.abs(out["Tcw"][k, :, 3] - np.array(S[1]) / S[2]).max() < 1e-14
    return out


def test_two_key_frames_one_edge():
    g = golden()
    out = device_run("two_kf")
    c = inputs("two_kf")
    S0 = R.from_record(c["Scw"][0])
    P0, P1 = R.from_record(c["Scw_prior"][0]), R.from_record(c["Scw_prior"][1])
    want = R.mul(R.mul(P1, R.inverse(P0)), S0)  # measurement^-1 * fixed pose
    d = max(R.pose_distance(R.from_record(out["Scw_opt"][1]), want))
    print("two_kf: chi2 %.3e -> %.3e (reference %.3e), distance to the closed form %.3e, %d trials" % (
        out["chi2_initial"], out["chi2_final"], float(g["two_kf/chi2_final"]), d, out["lm_trials"]))
    assert out["n_unknowns"] == 6 and out["chi2_initial"] == pytest.approx(float(g["two_kf/chi2_initial"]), rel=1e-12)
    # e is a rounding residue of log(C S1 S0^-1): 1e-15 * |t| per entry, chi2 below 1e-27; 1e-24 leaves three orders
    assert out["chi2_final"] < 1e-24
    assert d < 1e-12 and pose_errors("two_kf", out) < 1e-12
    assert np.array_equal(out["Scw_opt"][0:1].view(np.uint8), c["Scw"][0:1].view(np.uint8))  # the fixed vertex
    assert 1 <= out["lm_iterations"] <= N_ITERATIONS and out["lm_trials"] <= 10 * out["lm_iterations"]


def test_ring_of_24():
    out = check_against_golden("ring24")
    assert out["n_unknowns"] == 138


def test_ring_with_holes_and_a_fixed_key_frame_in_the_middle():
    out = check_against_golden("ring_holes")
    c = inputs("ring_holes")
    for k in (5, 17):  # invalid: Scw_opt is a copy, Tcw zeros
        assert np.array_equal(out["Scw_opt"][k:k + 1].view(np.uint8), c["Scw"][k:k + 1].view(np.uint8))
        assert not out["Tcw"][k].any()
    assert np.array_equal(out["Scw_opt"][11:12].view(np.uint8), c["Scw"][11:12].view(np.uint8))


def test_forty_key_frames_with_old_loops_covisibility_and_a_duplicate_edge():
    check_against_golden("kf40")


def test_free_scale():
    out = check_against_golden("scale16")
    assert out["n_unknowns"] == 105
    assert np.abs(out["Scw_opt"]["s"] - 1).max() > 1e-3  # the scale moves


def test_key_frame_without_an_edge_stays_bit_identical():
    out = check_against_golden("isolated")
    c = inputs("isolated")
    assert np.array_equal(out["Scw_opt"][24:25].view(np.uint8), c["Scw"][24:25].view(np.uint8))


def test_rejected_leading_trial_restores_and_grows_lambda():
    g = golden()
    out = check_against_golden("reject")
    lead = int(g["reject/n_leading"])
    rejected = np.flatnonzero(out["trace"]["accepted"][:lead] == 0)
    assert len(rejected) and rejected[0] + 1 < lead
    k = int(rejected[0])
    # a rejected trial leaves chi2_before as it was (the estimates were restored) and tries a larger lambda
    assert out["trace"]["chi2_before"][k + 1] == out["trace"]["chi2_before"][k]
    assert out["trace"]["lambda"][k + 1] == pytest.approx(2 * out["trace"]["lambda"][k], rel=1e-12)


def test_linearize_across_the_branches():
    g = golden()
    e, Ji, Jj = pg.linearize(**inputs("lin64"))
    de = np.abs(e - g["lin64/e"]).max()
    dj = np.maximum(np.abs(Ji - g["lin64/Ji"]).max(axis=(1, 2)), np.abs(Jj - g["lin64/Jj"]).max(axis=(1, 2)))
    ratio = dj / g["lin64/jac_spread"]
    print("lin64: |e - ref| max %.3e (bound 1e-12); Jacobian difference / recorded spread per edge: max %.2f at edge %d, "
          "median %.2f (bound 4)" % (de, ratio.max(), int(ratio.argmax()), float(np.median(ratio))))
    assert de < 1e-12
    assert (dj <= 4 * g["lin64/jac_spread"]).all(), np.flatnonzero(dj > 4 * g["lin64/jac_spread"])
    # under fix_scale the scale column is exactly zero
    c = inputs("lin64")
    c["fix_scale"] = True
    _, Ji, Jj = pg.linearize(**c)
    assert not Ji[:, :, 6].any() and not Jj[:, :, 6].any()


GEOMETRY_CHILD = """
import sys
import numpy as np
sys.path.insert(0, %r)
from tests import test_pose_graph as t
out = t.pg.optimize_essential_graph(**t.inputs("kf40"), Pw=t.ring_points(40)[0], ref_kf=t.ring_points(40)[1])
np.savez(sys.argv[1], Scw_opt=out["Scw_opt"], Tcw=out["Tcw"], Pw_out=out["Pw_out"], trace=out["trace"])
"""


def ring_points(n_kf, n=5000):
    rng = np.random.default_rng(5)
    Pw = (rng.standard_normal((n, 3)) * 6).astype(np.float32)
    ref = rng.integers(0, n_kf, n).astype(np.int32)
    ref[::17] = -1                 # bad points
    ref[1::5] = n_kf - 1 - (np.arange(len(ref[1::5])) % 3)  # the corrected key frames
    return Pw, ref


def test_determinism_across_calls_and_launch_geometry(tmp_path):
    Pw, ref = ring_points(40)
    a = pg.optimize_essential_graph(**inputs("kf40"), Pw=Pw, ref_kf=ref)
    b = pg.optimize_essential_graph(**inputs("kf40"), Pw=Pw, ref_kf=ref)
    for k in ("Scw_opt", "Tcw", "Pw_out", "trace"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    script = tmp_path / "alt.py"
    script.write_text(GEOMETRY_CHILD % ROOT)
    env = dict(os.environ, VIEO_PG_GEOMETRY="alt")
    subprocess.check_call([sys.executable, str(script), str(tmp_path / "alt.npz")], env=env, timeout=120)
    alt = np.load(tmp_path / "alt.npz")
    for k in ("Scw_opt", "Tcw", "Pw_out", "trace"):
        assert np.array_equal(a[k].view(np.uint8), np.ascontiguousarray(alt[k]).view(np.uint8)), k


def test_map_points():
    g = golden()
    c = inputs("ring24")
    Pw, ref = ring_points(24)
    # the kernel alone: no optimisation, the correction is Scw^-1 Scw
    rc, alone = pg.optimize_essential_graph_call(**c, Pw=Pw, ref_kf=ref, n_iterations=0, tap_points=True)
    assert rc == 0 and alone["lm_trials"] == 0
    Scw = [R.from_record(r) for r in c["Scw"]]
    _, want = R.finish(Scw, Scw, c["valid"], Pw, ref)
    rel = np.abs(alone["Pw_out_d"] - want).max(axis=1) / np.maximum(np.linalg.norm(Pw.astype(np.float64), axis=1), 1e-30)
    print("map points alone: worst relative difference before the cast %.3e (bound 1e-12)" % rel.max())
    assert rel.max() < 1e-12
    assert np.array_equal(alone["Pw_out"][ref < 0].view(np.uint8), Pw[ref < 0].view(np.uint8))
    assert np.array_equal(alone["Pw_out"], alone["Pw_out_d"].astype(np.float32))
    assert np.array_equal(alone["Scw_opt"].view(np.uint8), c["Scw"].view(np.uint8))
    # after the optimisation: against the reference's poses
    out = pg.optimize_essential_graph(**c, Pw=Pw, ref_kf=ref)
    _, want = R.finish([R.from_record(r) for r in sims(g["ring24/est"])], Scw, c["valid"], Pw, ref)
    d = np.abs(out["Pw_out"].astype(np.float64) - want).max()
    print("map points after the optimisation: worst difference %.3e m (bound 1e-4)" % d)
    assert d < 1e-4
    assert np.array_equal(out["Pw_out"][ref < 0].view(np.uint8), Pw[ref < 0].view(np.uint8))
    moved = np.abs(out["Pw_out"] - Pw).max(axis=1)
    assert moved[(ref >= 8) & (ref < 16)].max() > 1e-3  # mid-ring points are carried along with their key frames


def test_errors_leave_the_outputs_untouched():
    c = inputs("ring_holes")
    bad_edge = dict(c, edge_j=np.where(np.arange(len(c["edge_j"])) == 3, 5, c["edge_j"]))  # key frame 5 is invalid
    for args in (bad_edge, dict(c, fixed_kf=26), dict(c, fixed_kf=-1), dict(c, fixed_kf=17)):
        rc, out = pg.optimize_essential_graph_call(**args)
        assert rc == _lib.VIEO_E_INVALID
        assert out["status"] == -99 and (out["Scw_opt"]["s"] == -7.0).all() and (out["Tcw"] == -7.0).all()
    # no edge at all: succeeds, poses unchanged, points through the identity correction
    Pw, ref = ring_points(26)
    ref[(ref == 5) | (ref == 17)] = 0
    none = dict(c, edge_i=np.zeros(0, np.int32), edge_j=np.zeros(0, np.int32), edge_kind=np.zeros(0, np.int32),
                edge_info=np.zeros((0, 2)))
    rc, out = pg.optimize_essential_graph_call(**none, Pw=Pw, ref_kf=ref)
    assert rc == 0 and out["lm_trials"] == 0 and out["n_unknowns"] == 0
    assert np.array_equal(out["Scw_opt"].view(np.uint8), c["Scw"].view(np.uint8))
    assert np.array_equal(out["Pw_out"], Pw)
