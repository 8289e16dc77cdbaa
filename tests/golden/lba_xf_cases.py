"""The windows of tests/test_lba_xf_table.py: one shape per writer of the local BA's key-frame transform table.

Shared by the test and by make_lba_parent_golden.py, which records what the commit BEFORE the table (7423083) computed
for them on an MI355X (tests/golden/lba_parent_<case>.npz: states, points, erase flags, trial counts -- the table must
change none of their bytes).  Every window comes from synth_ba.make_lba_vio_problem.
"""
import numpy as np

from vieo_slam_amd import synth_ba

# case -> what runs it.  kind: "vio" LocalBundleAdjustmentNavStatePRV[Batch], "scale" the full BA with the scale vertex,
# "vision" the vision-only LocalBundleAdjustment on the same kind of window
SMALL = dict(seed=301, n_local=3, n_fixed=1, n_points=40)
CASES = {
    # 3 local + 1 fixed key frames, 40 points: k_lba_begin / k_lba_ldlt16 / k_lba_restore in a one-window call
    "small": dict(kind="vio", wins=[SMALL]),
    # 10 + 2 key frames, 200 points, gross outliers planted: k_lba_prelevel (the table's first writer), both
    # classifications, rejected and accepted trials
    "outliers": dict(kind="vio", wins=[dict(seed=346, n_local=10, n_fixed=2, n_points=200, plant=12)]),
    # bLarge at 11 local key frames = 165 unknowns, the smallest system of k_lba_ldltg's class (160 .. 639)
    "large": dict(kind="vio", wins=[dict(seed=303, n_local=11, n_fixed=2, n_points=300, dt_kf=0.25, large=True)]),
    # two distorted cameras per key frame: a table entry per (key frame, camera)
    "rig": dict(kind="vio", wins=[dict(seed=304, n_local=4, n_fixed=2, n_points=150, rig="radtan")]),
    # full BA with the scale vertex (EdgeReprojectPRS): the transform meets s * Xh
    "scale": dict(kind="scale", wins=[dict(seed=305, n_local=6, n_fixed=1, n_points=250, anchors=2)], s0=1.04, iters=6),
    # vision-only (pd = 6): only key frames with an active edge are free
    "vision": dict(kind="vision", wins=[dict(seed=306, n_local=5, n_fixed=2, n_points=150)]),
    # the small window in a call of 2 (the one-launch tail of a trial) and in a batch of 6 (the four-launch form)
    "pair": dict(kind="vio", wins=[SMALL, dict(seed=307, n_local=4, n_fixed=2, n_points=80)]),
    "six": dict(kind="vio", wins=[SMALL] + [dict(seed=308 + i, n_local=3 + i % 3, n_fixed=1 + i % 2, n_points=40 + 20 * i)
                                            for i in range(5)]),
}


def make_window(seed, plant=0, large=False, **kw):
    """(params, kfs, points, close, obs, imu) and the indices of the planted observations"""
    win = list(synth_ba.make_lba_vio_problem(seed, **kw)[:6])
    planted = np.zeros(0, np.int64)
    if plant:  # gross outliers: 150 px off is chi2 > 100 chi2_95 at every pyramid level (150^2 / 1.2^14 = 1752 > 781.5)
        obs = win[4].copy()
        planted = np.arange(plant) * (len(obs) // plant) + 3
        obs["u"][planted] += np.float32(150.0)
        win[4] = obs
    if large:
        P = win[0].copy()
        P[0]["large"], P[0]["lambda_init"] = 1, 1e-2
        P[0]["base"]["its0"], P[0]["base"]["its1"] = 2, 2
        win[0] = P
    return tuple(win), planted


def build(name):
    """the case's windows: list of ((params, kfs, points, close, obs, imu), planted)"""
    c = CASES[name]
    out = [make_window(**w) for w in c["wins"]]
    if c["kind"] == "scale":  # the map handed over divided by s0 (tests/test_global_ba_scale.py)
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
    """what a golden file keeps of a case's records"""
    out = {}
    for w, r in enumerate(recs):
        out["navs%d" % w] = np.frombuffer(np.ascontiguousarray(r["navs"]).tobytes(), np.uint8)
        out["pts%d" % w] = np.ascontiguousarray(r["pts"])
        out["erase%d" % w] = np.ascontiguousarray(r["erase"])
        out["trials%d" % w] = np.array([int(r["res"]["lm_trials"]), int(r["res"]["lm_iterations"]), int(r["res"]["status"])],
                                       np.int32)
        if r["scale"] is not None:
            out["scale%d" % w] = np.array([r["scale"]], np.float64)
    return out
