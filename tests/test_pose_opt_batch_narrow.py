"""The one-wavefront-per-frame PoseOptimization kernel (batches of more than 256 frames) with two wavefronts per SIMD and
eight frames per CU: same bytes as its parent, parity with the CPU oracle, no state shared between the frames of a CU.

One launch of 257 frames (tests/golden/pose_batch_narrow_cases.py) serves every test.  The parent's bytes are
tests/golden/pose_batch_narrow_parent.npz (recorded by tests/golden/make_pose_batch_narrow_golden.py)."""
import ctypes
import os

import numpy as np
import pytest

from tests.golden import pose_batch_narrow_cases as cases
from vieo_slam_amd import synth_ba

pytestmark = pytest.mark.gpu
TOL = 1e-4  # SE(3) parity bar of the pose optimisations (tests/test_pose_opt_vio_parity.py)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_batch_narrow_parent.npz")
FRAMES_PER_CU = 8  # profiles/pose_batch_occupancy.md


@pytest.fixture(scope="module")
def run():
    P, frames, obs = cases.build()
    res, outl = cases.run_hip(frames, obs)
    return P, frames, obs, res, outl


def _frame(run, i):
    _, frames, _, res, outl = run
    b, n = int(frames[i]["base"]["obs_begin"]), int(frames[i]["base"]["n_obs"])
    return res[i], outl[b:b + n]


def test_batch_takes_the_narrow_kernel_and_covers_the_cases(run):
    P, frames, obs, res, outl = run
    assert len(frames) == 257 and os.environ.get("VIEO_POSE_THREADS") != "256"  # (more than 256 frames: one wavefront each)
    n = sorted({int(F[0]["base"]["n_obs"]) for F, _, _ in P})
    assert set(n) >= {2, 3, 4, 63, 64, 65, 127, 128, 129, 600}
    for key in ("last_has_prior", "compute_marg"):
        assert {int(F[0][key]) for F, _, _ in P} == {0, 1}
    assert {bool(F[0]["imu"]["dt"] != 0) for F, _, _ in P} == {False, True}
    # the planted outliers are found (rounds reject edges), and a poor start costs rejected trials (the LM retry path)
    r, o = _frame(run, 2 + cases.NAMES.index("planted_outliers") - 1)
    gt = P[cases.NAMES.index("planted_outliers")][2]
    assert o.sum() >= 0.8 * gt["is_outlier"].sum() > 40
    rejected = [int(_frame(run, 2 + k - 1)[0]["base"]["reserved"]) - int(_frame(run, 2 + k - 1)[0]["base"]["lm_iterations"])
                for k, name in enumerate(cases.NAMES) if name.startswith("poor_start")]
    print("rejected trials of the poor starts:", rejected)
    assert max(rejected) > 0
    assert np.all(outl <= 1)  # every flag of every frame was written


def test_same_bytes_as_the_parent(run):
    g = np.load(GOLDEN)
    bad = []
    for i in range(cases.B):
        k = cases.which(i)
        r, o = _frame(run, i)
        f = cases.fields_of(r, o)
        for name in cases.FIELDS:
            if f[name] != g[name][k].tobytes():
                bad.append((i, cases.NAMES[k], name))
        b = int(g["outlier_len"][:k].sum())
        if f["outlier"] != g["outlier"][b:b + int(g["outlier_len"][k])].tobytes():
            bad.append((i, cases.NAMES[k], "outlier"))
    assert not bad, bad[:20]


@pytest.mark.parametrize("k", range(len(cases.NAMES)), ids=cases.NAMES)
def test_parity_with_the_oracle(run, oracle, k):
    P = run[0]
    F, obs, _ = P[k]
    i = cases.PROBE_POS[-1] if k == 0 else 2 + k - 1
    assert cases.which(i) == k
    h, ho = _frame(run, i)
    if cases.NAMES[k] == "too_few_2":  # Optimizer.h:499-503: nothing is optimised
        assert h["base"]["status"] == 1 and h["base"]["n_inliers"] == 0 and h["base"]["lm_iterations"] == 0
        assert h["has_marg"] == 0 and not h["H_marg"].any() and not ho.any()
        assert h["base"]["nav"].tobytes() == F[0]["base"]["nav"].tobytes()
        return
    o, oo = oracle.pose_optimization_vio(F, obs)
    dt, dr = synth_ba.pose_error(o["base"]["nav"], h["base"]["nav"])
    print(cases.NAMES[k], "dt %.2e dr %.2e" % (dt, dr), "inliers", int(o["base"]["n_inliers"]), int(h["base"]["n_inliers"]))
    assert dt < TOL and dr < TOL, (dt, dr)
    assert np.linalg.norm(o["base"]["nav"]["v"] - h["base"]["nav"]["v"]) < 1e-4
    assert np.linalg.norm(o["base"]["nav"]["dbg"] - h["base"]["nav"]["dbg"]) < 1e-6
    assert np.linalg.norm(o["base"]["nav"]["dba"] - h["base"]["nav"]["dba"]) < 1e-5
    assert o["base"]["status"] == h["base"]["status"] == 0
    assert o["base"]["n_inliers"] == h["base"]["n_inliers"]
    assert np.array_equal(oo, ho)
    assert o["has_marg"] == h["has_marg"] == F[0]["compute_marg"]
    if o["has_marg"]:
        rtol = 1e-4 if F[0]["last_has_prior"] else 1e-5  # (as the parity tests of the two forms)
        Ho, Hh = o["H_marg"].reshape(15, 15), h["H_marg"].reshape(15, 15)
        assert np.allclose(Ho, Hh, rtol=rtol, atol=rtol * np.abs(Ho).max())
    else:
        assert not h["H_marg"].any()


def test_same_frame_at_four_positions(run):
    """State shared between the workgroups of a CU (eight of them in its LDS now) would show as a frame whose result
    depends on its neighbours."""
    ref = cases.fields_of(*_frame(run, cases.PROBE_POS[0]))
    for i in cases.PROBE_POS[1:]:
        f = cases.fields_of(*_frame(run, i))
        assert [name for name in f if f[name] != ref[name]] == [], i
    # ... and so would any other problem: every repeat in the batch equals its first occurrence
    first = {}
    for i in range(cases.B):
        f = cases.fields_of(*_frame(run, i))
        assert first.setdefault(cases.which(i), f) == f, (i, cases.NAMES[cases.which(i)])


def test_frames_per_cu():
    from vieo_slam_amd._lib import lib
    fn = lib().vieo_debug_pose_vio_batch_residency
    fn.restype, fn.argtypes = ctypes.c_int, []
    n = int(fn())
    print("frames per CU:", n)
    assert n >= FRAMES_PER_CU and n >= 5
