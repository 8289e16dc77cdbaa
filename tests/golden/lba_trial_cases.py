"""The windows of tests/test_lba_trial_round.py: the smallest shapes at which the per-trial round of the local BA can go
wrong -- which 16 x 16 blocks of a diagonal Schur tile k_lba_schur computes (lba_schur_device.h), and what the solves gather.

Shared by the test and by make_lba_trial_golden.py, which records what the commit BEFORE both changes computed for
them on an MI355X (tests/golden/lba_trial_<case>.npz).  The windows are built as in lba_xf_cases (make_window).

Point counts: make_lba_vio_problem drops the points too few key frames see; N_POINTS is what is left, and the test pins
it.  Only vis11's 96 is a multiple of 16: every other window ends in a ragged chunk (40 = 2 x 16 + 8, 63 = 3 x 16 + 15,
...).  A split of the Schur product that owns no chunk (split * cps >= chunks, the kernel's early return) cannot occur
in a local window of 40 .. 200 points: its ksplit = ceil(chunks / 8) gives every split a chunk.  The full BA takes
ksplit = min(chunks, 16), so the scale case has 267 points = 17 chunks: cps = 2, nine splits work and seven return at
once.
"""
import numpy as np

from tests.golden import lba_xf_cases as xf

# case -> what runs it (kinds as in lba_xf_cases).  npv: rows of the visual system, n: unknowns of the reduced system.
KF3 = dict(seed=413, n_local=3, n_fixed=1, n_points=72)
LARGE11 = dict(seed=419, n_local=11, n_fixed=2, n_points=200, dt_kf=0.25, large=True)
CASES = {
    # where column npv (b_l) falls in the one diagonal tile: npv = 6, 12, 18, 36, 48, 60 -> column block 0, 0, 1, 2, 3, 3,
    # padding row blocks 3, 3, 2, 1, 1, 0; n = 15 .. 150 in k_lba_ldlt16.  One window each: fused build, k_lba_tail.
    "kf1": dict(kind="vio", wins=[dict(seed=411, n_local=1, n_fixed=2, n_points=130)]),
    "kf2": dict(kind="vio", wins=[dict(seed=412, n_local=2, n_fixed=2, n_points=130)]),
    "kf3": dict(kind="vio", wins=[KF3]),
    "kf6": dict(kind="vio", wins=[dict(seed=414, n_local=6, n_fixed=2, n_points=104)]),
    "kf8": dict(kind="vio", wins=[dict(seed=415, n_local=8, n_fixed=2, n_points=150)]),
    # npv = 60 with gross outliers planted (lba_xf_cases "outliers"): a rejected trial is a new lambda on an unchanged
    # build -- assembly with only lambda changed -- then the restore
    "kf10": dict(kind="vio", wins=[dict(seed=346, n_local=10, n_fixed=2, n_points=200, plant=12)]),
    # more than one tile in class 0, vision-only (pd = 6).  11 key frames: npv = 66, a second diagonal tile with two
    # valid rows and column npv in its block 0, one off-diagonal tile.  26: npv = n = 156, the largest class-0 system.
    "vis11": dict(kind="vision", wins=[dict(seed=417, n_local=11, n_fixed=2, n_points=120)]),
    "vis26": dict(kind="vision", wins=[dict(seed=418, n_local=26, n_fixed=2, n_points=200, dt_kf=0.1)]),
    # class 1 (k_lba_ldltg): 11 key frames of a visual-inertial window, n = 165, two diagonal tiles
    "large11": dict(kind="vio", wins=[LARGE11]),
    # the scale vertex: row / column npv - 1 = 36 of the visual system, H_ps / H_ss in lba_assemble_entry; 17 chunks
    "scale": dict(kind="scale", wins=[dict(seed=420, n_local=6, n_fixed=1, n_points=440, anchors=2)], s0=1.04, iters=6),
    # kf3 first of six, a class-0 / class-1 mix: separate launches, one assembly loop per class
    "six": dict(kind="vio", wins=[KF3, LARGE11] + [dict(seed=421 + i, n_local=2 + 2 * i, n_fixed=1 + i % 2, n_points=48 + 24 * i)
                                                   for i in range(4)]),
}

# points left per window of the case (see above)
N_POINTS = {"kf1": [66], "kf2": [63], "kf3": [40], "kf6": [69], "kf8": [120], "kf10": [124], "vis11": [96], "vis26": [122],
            "large11": [124], "scale": [267], "six": [40, 124, 20, 41, 65, 85]}


def build(name):
    """the case's windows: list of ((params, kfs, points, close, obs, imu), planted)"""
    c = CASES[name]
    out = [xf.make_window(**w) for w in c["wins"]]
    if c["kind"] == "scale":  # the map handed over divided by s0, as in lba_xf_cases
        out = [((w[0], w[1], (w[2] / np.float32(c["s0"])).astype(np.float32)) + w[3:], p) for w, p in out]
    return out


def _rec(navs, pts, erase, res, scale=None):
    return dict(navs=navs, pts=pts, erase=erase, res=res, scale=scale)


def run_hip(name, wins):
    """the case on the device: one record per window"""
    from vieo_slam_amd.optimizer import Optimizer
    c = CASES[name]
    if c["kind"] == "vio":
        if len(wins) == 1:
            return [_rec(*Optimizer.LocalBundleAdjustmentNavStatePRV(*wins[0][0]))]
        return [_rec(*r) for r in Optimizer.LocalBundleAdjustmentNavStatePRVBatch([w for w, _ in wins])]
    (params, kfs, pts, close, obs, imu), _ = wins[0]
    if c["kind"] == "scale":
        n, p, r, s = Optimizer.GlobalBundleAdjustmentNavStatePRV(params, kfs, pts, obs, imu, c["iters"], True, bScaleOpt=True)
        return [_rec(n, p, np.zeros(0, np.uint8), r, s)]
    return [_rec(*Optimizer.LocalBundleAdjustment(params["base"], kfs, pts, obs))]


def run_oracle(oracle, name, wins):
    c = CASES[name]
    if c["kind"] == "vio":
        return [_rec(*oracle.local_ba_vio(*w)) for w, _ in wins]
    (params, kfs, pts, close, obs, imu), _ = wins[0]
    if c["kind"] == "scale":
        n, p, r, s = oracle.global_ba_vio(params, kfs, pts, obs, imu, c["iters"], True, scale_opt=True)
        return [_rec(n, p, np.zeros(0, np.uint8), r, s)]
    return [_rec(*oracle.local_ba(params["base"], kfs, pts, obs))]


def pack(recs):
    """what a golden file keeps of a case's records: lba_xf_cases.pack and chi2 (initial, final) per window"""
    out = xf.pack(recs)
    for w, r in enumerate(recs):
        out["chi2_%d" % w] = np.array([r["res"]["chi2_initial"], r["res"]["chi2_final"]], np.float64)
    return out
