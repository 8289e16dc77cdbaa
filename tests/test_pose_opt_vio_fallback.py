"""k_pose_opt_vio through the plain-form fallback of its single-lane edges (csrc/vio_fast_device.h): frames whose
first evaluations lie outside the polynomial domains of imu_error_rot, prior_error, ns_inc_unit and imu_linearize_rot,
which no tracked-sequence test reaches (the largest start elsewhere is 8 degrees).  Each about 150 observations, through
the four-wavefront instance here and through the one-wavefront instance in a fresh process (VIEO_POSE_THREADS is read
once), both within the 1e-4 SE(3) bar of the CPU oracle.

  start_35deg          the current state starts 35 degrees (0.61 rad > 0.49) from the IMU prediction: the first
                       evaluations of the inertial edge and the first retractions take the plain forms, the later ones
                       the polynomials
  start_35deg_prior    the same with a free last state that itself starts 35 degrees from its prior: prior_error too
  bias_correction      |JgR dbg_i| = 0.55 rad (half a second between the frames, a gyroscope bias correction of
                       1.1 rad / s on the fixed last state, the measurement made consistent with it): w_small is false in
                       every evaluation, Jr(w) comes from so3_Jr_d

The seeds are ones at which the CPU oracle converges to the scene's truth (asserted); at 35 degrees each of the 12
tried did, so the angle was not reduced."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.golden.pose_batch_narrow_cases import _prior_info
from vieo_slam_amd import synth_ba

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4  # SE(3) parity bar of the pose optimisations (tests/test_pose_opt_vio_parity.py)
START = np.deg2rad(35.0)
NAMES = ("start_35deg", "start_35deg_prior", "bias_correction")


def _axis(seed):
    a = np.random.default_rng(seed).normal(0, 1, 3)
    return a / np.linalg.norm(a)


def frames():
    out = []
    F, obs, gt = synth_ba.make_vio_problem(900, n_obs=150, outlier_frac=0.05)
    F[0]["base"]["nav"]["q"] = synth_ba.quat_mul(gt["q"], synth_ba.quat_from_rotvec(START * _axis(905)))
    out.append((F, obs, gt))
    F1, _, _ = synth_ba.make_vio_problem(901, n_obs=150, outlier_frac=0.05)
    nav_prior = F1[0]["nav_last"].copy()
    nav_last = nav_prior.copy()
    nav_last["q"] = synth_ba.quat_mul(nav_prior["q"], synth_ba.quat_from_rotvec(START * _axis(906)))
    F, obs, gt = synth_ba.make_vio_problem(901, n_obs=150, outlier_frac=0.05, prior=(nav_prior, _prior_info(), nav_last))
    F[0]["base"]["nav"]["q"] = synth_ba.quat_mul(gt["q"], synth_ba.quat_from_rotvec(START * _axis(907)))
    out.append((F, obs, gt))
    F, obs, gt = synth_ba.make_vio_problem(902, n_obs=150, outlier_frac=0.05, dt_frame=0.5)
    im = F[0]["imu"]
    JgR = im["JgR"].reshape(3, 3)
    d = _axis(908)
    d *= 0.55 / np.linalg.norm(JgR @ d)
    F[0]["nav_last"]["dbg"] = d
    im["Rij"] = (im["Rij"].reshape(3, 3) @ synth_ba.so3_exp(JgR @ d).T).reshape(-1)
    im["vij"] = im["vij"] - im["Jgv"].reshape(3, 3) @ d
    im["pij"] = im["pij"] - im["Jgp"].reshape(3, 3) @ d
    out.append((F, obs, gt))
    return out


def run_hip():
    from vieo_slam_amd.optimizer import Optimizer
    return [Optimizer.PoseOptimizationVIO(F, obs) for F, obs, _ in frames()]


@pytest.fixture(scope="module")
def hip_results():
    return run_hip()


@pytest.fixture(scope="module")
def oracle_results(oracle):
    return [oracle.pose_optimization_vio(F, obs) for F, obs, _ in frames()]


def test_frames_start_outside_the_domains_and_the_oracle_finds_the_truth(oracle_results):
    P = frames()
    for k, (F, obs, gt) in enumerate(P):
        assert 140 <= len(obs) <= 160
        o, _ = oracle_results[k]
        dt = float(np.linalg.norm(o["base"]["nav"]["p"] - gt["p"]))
        dr = 2 * np.arccos(min(1.0, abs(float(np.dot(o["base"]["nav"]["q"], gt["q"])))))
        print(NAMES[k], "oracle against the truth: dt %.2e dr %.2e, %d LM iterations" % (dt, dr, int(o["base"]["lm_iterations"])))
        assert o["base"]["status"] == 0 and dt < 0.01 and dr < 2e-3, (NAMES[k], dt, dr)
    for k in (0, 1):
        nav, gt = P[k][0][0]["base"]["nav"], P[k][2]
        assert 2 * np.arccos(abs(float(np.dot(nav["q"], gt["q"])))) > 0.6
    F = P[1][0][0]
    assert F["last_has_prior"] == 1 and 2 * np.arccos(abs(float(np.dot(F["nav_last"]["q"], F["nav_prior"]["q"])))) > 0.6
    F = P[2][0][0]
    assert np.linalg.norm(F["imu"]["JgR"].reshape(3, 3) @ F["nav_last"]["dbg"]) > 0.5 and F["last_has_prior"] == 0


def _compare(o, oo, h, ho, name):
    dt, dr = synth_ba.pose_error(o["base"]["nav"], h["base"]["nav"])
    print(name, "dt %.2e dr %.2e" % (dt, dr), "inliers", int(o["base"]["n_inliers"]), int(h["base"]["n_inliers"]))
    assert dt < TOL and dr < TOL, (name, dt, dr)
    assert np.linalg.norm(o["base"]["nav"]["v"] - h["base"]["nav"]["v"]) < 1e-4
    assert np.linalg.norm(o["base"]["nav"]["dbg"] - h["base"]["nav"]["dbg"]) < 1e-6
    assert np.linalg.norm(o["base"]["nav"]["dba"] - h["base"]["nav"]["dba"]) < 1e-5
    assert o["base"]["status"] == h["base"]["status"] == 0
    assert o["base"]["n_inliers"] == h["base"]["n_inliers"] and np.array_equal(oo, ho)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(NAMES)), ids=NAMES)
def test_four_wavefronts_per_frame(oracle_results, hip_results, k):
    assert os.environ.get("VIEO_POSE_THREADS") != "64"
    h, ho = hip_results[k]
    _compare(*oracle_results[k], h, ho, NAMES[k])


CHILD = """
import sys
import numpy as np
sys.path.insert(0, %r)
from tests import test_pose_opt_vio_fallback as t
res = t.run_hip()
np.savez(sys.argv[1], res=np.array([r for r, _ in res]), **{"outl%%d" %% k: o for k, (_, o) in enumerate(res)})
"""


@pytest.mark.gpu
def test_one_wavefront_per_frame(oracle_results, tmp_path):
    script = tmp_path / "narrow.py"
    script.write_text(CHILD % ROOT)
    env = dict(os.environ, VIEO_POSE_THREADS="64")
    subprocess.check_call([sys.executable, str(script), str(tmp_path / "narrow.npz")], env=env, timeout=120)
    got = np.load(tmp_path / "narrow.npz")
    for k, name in enumerate(NAMES):
        _compare(*oracle_results[k], got["res"][k], got["outl%d" % k], name + " (64 threads)")
