"""The full BA's tile-sparse LDL^T (solver class 3, gba_sparse_plan.h) on the GPU: full BAs past the dense solve's
16320-unknown cap, and byte-identity with the dense tiled solve (k_big_*) on the same problems.

VIEO_LBA_SPARSE_SOLVE / VIEO_LBA_BIG_SOLVE are read once per process: the forced runs go to child processes."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from vieo_slam_amd import synth_ba

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gt_err(navs, gt, n):
    dp = np.linalg.norm(navs["p"][:n] - gt["p"][:n], axis=1)
    dr = np.array([synth_ba.pose_error(navs[k], dict(p=navs[k]["p"], q=gt["q"][k]))[1] for k in range(n)])
    return dp, dr


def _launches(times):
    return {k: v["launches"] for k, v in times.items()}


# ---- the problems of the forced runs (seeded: the child processes build the same ones)
def _p400():
    params, kfs, pts, close, obs, imu, gt = synth_ba.make_lba_vio_problem(7, n_local=400, n_fixed=1, n_points=4000,
                                                                          anchors=200, span=5)
    return params, kfs, (pts / np.float32(1.02)).astype(np.float32), obs, imu


def _runs():
    """name -> callable returning (navs, points, result record, scale)"""
    from vieo_slam_amd.optimizer import Optimizer

    def vio(win, iters, robust):
        params, kfs, pts, obs, imu = win
        return lambda: Optimizer.GlobalBundleAdjustmentNavStatePRV(params, kfs, pts, obs, imu, iters, robust, bScaleOpt=True)

    def vis(win, iters, robust, stop=None):
        P, kfs, pts, obs, gt = win
        return lambda: Optimizer.BundleAdjustment(P, kfs, pts, obs, iters, robust, stop=stop) + (1.0,)

    loop = synth_ba.make_lba_vio_problem(23, n_local=60, n_fixed=1, n_points=3000, anchors=30, span=5, loop=40)
    v500 = synth_ba.make_lba_problem(24, n_local=500, n_fixed=1, n_points=8000, anchors=250, span=5, loop=20)
    return {
        "vio400_scale": vio(_p400(), 2, True),
        "vio60_loop": vio((loop[0], loop[1], loop[2], loop[4], loop[5]), 6, True),
        "vision500_robust": vis(v500, 5, True),
        "vision500_plain": vis(v500, 5, False),
        "vision500_stop": vis(v500, 5, True, stop=np.ones(1, np.int32)),
    }


def _child(out_path):
    """runs every problem of _runs() under this process's solver setting, writes the outputs and launch counts"""
    from vieo_slam_amd.optimizer import Optimizer
    res = {}
    for name, fn in _runs().items():
        Optimizer.enable_kernel_timing(2)
        navs, pts, rec, scale = fn()
        lc = _launches(Optimizer.kernel_times()[0])
        res[name + ".navs"] = np.frombuffer(navs.tobytes(), np.uint8)
        res[name + ".pts"] = np.frombuffer(pts.tobytes(), np.uint8)
        res[name + ".rec"] = np.frombuffer(np.asarray(rec).tobytes(), np.uint8)
        res[name + ".scale"] = np.frombuffer(np.float64(scale).tobytes(), np.uint8)
        res[name + ".ldlt"] = np.array([lc["lba.ldlt"], lc["lba.ldlt_sparse"]])
    Optimizer.enable_kernel_timing(0)
    np.savez(out_path, **res)


def _run_child(env_var, tmp):
    out = os.path.join(tmp, env_var + ".npz")
    env = dict(os.environ, **{env_var: "1"})
    env.pop("VIEO_LBA_SPARSE_SOLVE" if env_var == "VIEO_LBA_BIG_SOLVE" else "VIEO_LBA_BIG_SOLVE", None)
    subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); from tests import test_gba_sparse as t; "
                    "t._child(%r)" % (ROOT, out)], cwd=ROOT, env=env, check=True, timeout=600)
    return dict(np.load(out))


@pytest.fixture(scope="module")
def forced_runs():
    with tempfile.TemporaryDirectory() as tmp:
        return _run_child("VIEO_LBA_SPARSE_SOLVE", tmp), _run_child("VIEO_LBA_BIG_SOLVE", tmp)


# ------------------------------------------------------------------ byte-identity with the dense tiled solve
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["vio400_scale", "vio60_loop", "vision500_robust", "vision500_plain", "vision500_stop"])
def test_sparse_solve_byte_identical_to_dense_tiled_solve(forced_runs, name):
    """Forced tile-sparse against forced dense tiled solve, same problem: navs, points, result record and scale agree
    to the byte.  (A tile outside the fill pattern only contributes exact zeros to the dense factorisation; the sparse
    path skips it.  The one difference this could make is the sign of an exact zero in back-substitution; none appears.)"""
    sp, de = forced_runs
    for part in ("navs", "pts", "rec", "scale"):
        assert np.array_equal(sp[name + "." + part], de[name + "." + part]), part
    ldlt_sp, ldlt_de = sp[name + ".ldlt"], de[name + ".ldlt"]
    if name.endswith("stop"):  # the stop flag ends both before any solve
        assert ldlt_sp.sum() == 0 and ldlt_de.sum() == 0
        rec = np.frombuffer(sp[name + ".rec"].tobytes(), dtype=synth_ba_result_dtype())
        assert rec["status"][0] == 1
    else:
        assert ldlt_sp[0] == 0 and ldlt_sp[1] > 0, ldlt_sp
        assert ldlt_de[0] > 0 and ldlt_de[1] == 0, ldlt_de


def synth_ba_result_dtype():
    from vieo_slam_amd.ba_types import LBA_RESULT_DTYPE
    return LBA_RESULT_DTYPE


@pytest.mark.gpu
def test_sparse_solve_400_key_frames_matches_oracle(forced_runs, oracle):
    """The forced tile-sparse 400-key-frame call against the oracle, as test_vio_gba_scale_400_key_frames_parity checks
    the dense one."""
    from vieo_slam_amd.ba_types import NAVSTATE_DTYPE
    params, kfs, pts, obs, imu = _p400()
    on, op, ores, osc = oracle.global_ba_vio(params, kfs, pts, obs, imu, 2, True, scale_opt=True)
    sp = forced_runs[0]
    hn = np.frombuffer(sp["vio400_scale.navs"].tobytes(), NAVSTATE_DTYPE)
    hsc = float(np.frombuffer(sp["vio400_scale.scale"].tobytes(), np.float64)[0])
    dt = np.linalg.norm(on["p"][:400] - hn["p"][:400], axis=1).max()
    dr = max(synth_ba.pose_error(on[k], hn[k])[1] for k in range(400))
    assert dt < 1e-4 and dr < 1e-4, (dt, dr)
    assert abs(osc - hsc) < 1e-6, (osc, hsc)


# ------------------------------------------------------------------ past the dense cap
@pytest.fixture(scope="module")
def vio2000():
    return synth_ba.make_lba_vio_problem(31, n_local=2000, n_fixed=1, n_points=10000, anchors=1000, span=5,
                                         outlier_frac=0.0, noise=0.0, stereo_frac=1.0, imu_noise=0.0)


@pytest.mark.gpu
def test_vio_gba_scale_2000_key_frames_noiseless(vio2000):
    """2 000 free visual-inertial key frames with the scale vertex: 30 001 unknowns, past the dense solve's 16 320 (it
    returned VIEO_E_CAPACITY).  Noiseless observations (rounded to float): the truth within the tolerances of
    test_oracle_vio_gba_noiseless_recovers_truth, the scale within 5e-3; the tile-sparse solve ran and the dense one did
    not; a second call gives the same bytes.
    60 iterations, map at scale 1: this trajectory is 3.8 km long, and on it LM needs more than 20 iterations (at 20 the
    worst key frame is 5.6 mm off); a map handed over 2 % small is tens of metres off at that distance, which 60
    iterations do not recover either -- on 400 key frames of the same generator the dense tiled solve behaves the same."""
    from vieo_slam_amd.optimizer import Optimizer
    params, kfs, pts, close, obs, imu, gt = vio2000
    Optimizer.enable_kernel_timing(2)
    hn, hp, hres, hsc = Optimizer.GlobalBundleAdjustmentNavStatePRV(params, kfs, pts, obs, imu, 60, False, bScaleOpt=True)
    lc = _launches(Optimizer.kernel_times()[0])
    Optimizer.enable_kernel_timing(0)
    assert hres["status"] == 0
    assert lc["lba.ldlt_sparse"] > 0 and lc["lba.ldlt"] == 0, lc
    dp, dr = _gt_err(hn, gt, 2000)
    assert dp.max() < 1e-3 and dr.max() < 2e-4, (dp.max(), dr.max())
    assert abs(hsc - 1.0) < 5e-3, hsc
    hn2, hp2, hres2, hsc2 = Optimizer.GlobalBundleAdjustmentNavStatePRV(params, kfs, pts, obs, imu, 60, False, bScaleOpt=True)
    assert hn.tobytes() == hn2.tobytes() and hp.tobytes() == hp2.tobytes() and hsc == hsc2
    assert np.asarray(hres).tobytes() == np.asarray(hres2).tobytes()


def _with_pixel_noise(obs, seed):
    """1-pixel Gaussian noise (x the level's sigma) on the observations of a noiseless problem, 3 % of them 40-pixel
    outliers (the problem generator's noise model, without generating the inertial chain again)"""
    rng = np.random.default_rng(seed)
    o = obs.copy()
    sig = 1.0 / np.sqrt(o["inv_sigma2"].astype(np.float64))
    for f in ("u", "v"):
        o[f] += (rng.normal(0, 1, len(o)) * sig).astype(np.float32)
    st = o["ur"] >= 0
    o["ur"][st] += (rng.normal(0, 1, st.sum()) * sig[st]).astype(np.float32)
    out = rng.random(len(o)) < 0.03
    o["u"][out] += rng.uniform(-40, 40, out.sum()).astype(np.float32)
    return o


@pytest.mark.gpu
def test_vio_gba_scale_2000_key_frames_noisy(vio2000):
    """Noisy 2 000-key-frame map: the cost goes down and the poses are as close to the truth as on a 400-key-frame map
    with the same noise (dense tiled solve) -- median errors, within 1.5 x: the longer chain has more room to drift.
    (Map at scale 1 and 60 iterations, see the noiseless test.)"""
    from vieo_slam_amd.optimizer import Optimizer
    p400 = synth_ba.make_lba_vio_problem(31, n_local=400, n_fixed=1, n_points=2000, anchors=200, span=5,
                                         outlier_frac=0.0, noise=0.0, stereo_frac=1.0, imu_noise=0.0)
    errs = []
    for n_local, (params, kfs, pts, close, obs, imu, gt) in ((400, p400), (2000, vio2000)):
        obs = _with_pixel_noise(obs, n_local)
        hn, hp, hres, hsc = Optimizer.GlobalBundleAdjustmentNavStatePRV(params, kfs, pts, obs, imu, 60, True, bScaleOpt=True)
        assert hres["status"] == 0 and hres["chi2_final"] < hres["chi2_initial"]
        dp, dr = _gt_err(hn, gt, n_local)
        errs.append((np.median(dp), np.median(dr)))
    assert errs[1][0] <= 1.5 * errs[0][0] and errs[1][1] <= 1.5 * errs[0][1], errs


@pytest.mark.gpu
def test_vision_gba_3000_key_frames_noiseless():
    """BundleAdjustment over 3 000 free key frames (18 000 unknowns, past the dense cap): VIEO_OK and the truth
    (60 iterations: a long chain, see the VIO test)."""
    from vieo_slam_amd.optimizer import Optimizer
    P, kfs, pts, obs, gt = synth_ba.make_lba_problem(33, n_local=3000, n_fixed=1, n_points=15000, anchors=1500, span=5,
                                                     outlier_frac=0.0, noise=0.0, stereo_frac=1.0)
    Optimizer.enable_kernel_timing(2)
    hn, hp, hres = Optimizer.BundleAdjustment(P, kfs, pts, obs, 60, False)
    lc = _launches(Optimizer.kernel_times()[0])
    Optimizer.enable_kernel_timing(0)
    assert hres["status"] == 0 and lc["lba.ldlt_sparse"] > 0 and lc["lba.ldlt"] == 0, (hres, lc)
    dp, dr = _gt_err(hn, gt, 3000)
    assert dp.max() < 1e-3 and dr.max() < 2e-4, (dp.max(), dr.max())


@pytest.mark.gpu
def test_sparse_call_past_the_cap_stops_on_the_stop_flag(vio2000):
    """The stop flag ends a call past the cap as it ends a dense one: status 1, the inputs returned."""
    from vieo_slam_amd.optimizer import Optimizer
    params, kfs, pts, close, obs, imu, gt = vio2000
    hn, hp, hres, hsc = Optimizer.GlobalBundleAdjustmentNavStatePRV(params, kfs, pts, obs, imu, 5, True, bScaleOpt=True,
                                                                    stop=np.ones(1, np.int32))
    assert hres["status"] == 1 and np.array_equal(hn["p"], kfs["nav"]["p"]) and np.array_equal(hp, pts) and hsc == 1.0
