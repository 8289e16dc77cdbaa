"""The batch of tests/test_pose_opt_batch_narrow.py and of its recorder (make_pose_batch_narrow_golden.py): 257 frames
-- one more than the largest batch that still takes the four-wavefront kernel -- made of 15 distinct problems.

Problem 0 (the "probe": 129 edges, free last state with a prior, marginalisation) sits at the batch positions 0, 1, 255
and 256, the others fill the positions between in turn, so the probe meets different neighbours on its compute unit.
"""
import numpy as np

from vieo_slam_amd import synth_ba
from vieo_slam_amd.ba_types import VIO_FRAME_DTYPE, VIO_RESULT_DTYPE

B = 257
PROBE_POS = (0, 1, 255, 256)
FIELDS = ("nav", "n_inliers", "status", "lm_iterations", "lm_trials", "H_marg", "has_marg")


def _prior_info():
    """A 15 x 15 information matrix of the last state (p, v, Phi, bg, ba) from integers: the same bits everywhere."""
    d = np.array([1e4] * 3 + [1e3] * 3 + [1e4] * 3 + [1e6] * 3 + [1e4] * 3)
    u = np.array([1, -2, 3, 1, 0, -1, 2, 1, -3, 4, -1, 2, 0, 3, -2], np.float64)
    return np.diag(d) + 16.0 * np.outer(u, u)


# name -> (seed, make_vio_problem keywords, free last state with a prior?, drop the IMU edge?)
SPECS = [
    ("probe_129_prior_marg", 700, dict(n_obs=129, compute_marg=True), True, False),
    ("min_3", 701, dict(n_obs=3, outlier_frac=0.0), False, False),
    ("n_4_marg", 702, dict(n_obs=4, outlier_frac=0.0, compute_marg=True), False, False),
    ("n_63_prior", 703, dict(n_obs=63), True, False),
    ("n_64_no_imu_marg", 704, dict(n_obs=64, compute_marg=True), False, True),
    ("n_65", 705, dict(n_obs=65), False, False),
    ("n_127_prior_marg", 706, dict(n_obs=127, compute_marg=True), True, False),
    ("n_128_marg", 707, dict(n_obs=128, compute_marg=True), False, False),
    ("n_129", 708, dict(n_obs=129), False, False),
    ("n_600_prior_marg", 709, dict(n_obs=600, compute_marg=True), True, False),
    ("too_few_2", 710, dict(n_obs=2, compute_marg=True), False, False),
    ("planted_outliers", 711, dict(n_obs=200, outlier_frac=0.35, compute_marg=True), False, False),
    ("poor_start", 712, dict(n_obs=150, pert_t=0.5, pert_r_deg=8.0), False, False),
    ("poor_start_prior", 713, dict(n_obs=150, pert_t=0.3, pert_r_deg=5.0, compute_marg=True), True, False),
    ("rescue_40", 714, dict(n_obs=40, outlier_frac=0.5, compute_marg=True), False, False),
]
NAMES = [s[0] for s in SPECS]


def protos():
    out = []
    for name, seed, kw, prior, no_imu in SPECS:
        kw = dict(kw)
        if prior:
            F1, _, _ = synth_ba.make_vio_problem(seed, **kw)
            nav_last = F1[0]["nav_last"].copy()
            nav_prior = nav_last.copy()
            nav_last["p"] += 0.004
            nav_last["v"] += 0.015
            kw["prior"] = (nav_prior, _prior_info(), nav_last)
        F, obs, gt = synth_ba.make_vio_problem(seed, **kw)
        if no_imu:
            F[0]["imu"]["dt"] = 0
        out.append((F, obs, gt))
    return out


def which(pos):
    """batch position -> problem"""
    return 0 if pos in PROBE_POS else 1 + (pos - 2) % (len(SPECS) - 1)


def build():
    P = protos()
    frames = np.zeros(B, VIO_FRAME_DTYPE)
    all_obs, begin = [], 0
    for i in range(B):
        F, obs, _ = P[which(i)]
        frames[i] = F[0]
        frames[i]["base"]["obs_begin"] = begin
        begin += len(obs)
        all_obs.append(obs)
    return P, frames, np.concatenate(all_obs)


def run_hip(frames, obs):
    """one launch of the batch entry; (results[B], outlier bytes)"""
    from vieo_slam_amd._lib import DeviceBuffer, check, lib
    dF, dO = DeviceBuffer(frames.nbytes), DeviceBuffer(obs.nbytes)
    dU, dR = DeviceBuffer(len(obs)), DeviceBuffer(B * VIO_RESULT_DTYPE.itemsize)
    dF.upload(frames)
    dO.upload(obs)
    dU.upload(np.full(len(obs), 0xEE, np.uint8))  # (a flag the kernel must write shows if it did not)
    check(lib().vieo_pose_optimization_vio_batch_device_ex(dF.ptr, B, dO.ptr, dU.ptr, dR.ptr, 1, 1, None))
    check(lib().vieo_device_synchronize())
    return dR.download(VIO_RESULT_DTYPE, (B,)), dU.download(np.uint8, (len(obs),))


def fields_of(res, outl):
    """the compared fields of one frame's result as byte strings"""
    return {"nav": res["base"]["nav"].tobytes(), "n_inliers": res["base"]["n_inliers"].tobytes(),
            "status": res["base"]["status"].tobytes(), "lm_iterations": res["base"]["lm_iterations"].tobytes(),
            "lm_trials": res["base"]["reserved"].tobytes(), "H_marg": res["H_marg"].tobytes(),
            "has_marg": res["has_marg"].tobytes(), "outlier": outl.tobytes()}
