"""The map of replay.Replay -- observation table, window of the local BA, its write-back -- on a hand-built map: 3 key frames
x 6 keys, 5 points, under both observation rules (one_key_per_kf: a key frame's second key replaces the first / the keys
are a sorted set) and with the mode's data (inertial or not, rectified pair or camera table).  No GPU, no oracle: the stages
object is a fake whose local BA returns its inputs plus chosen erase flags."""
import numpy as np
import pytest

from vieo_slam_amd import replay, replay_modes as rm, synth_ba
from vieo_slam_amd.ba_types import (CAMERA_DTYPE, IMU_PREINT_DTYPE, LBA_PARAMS_DTYPE, LBA_RESULT_DTYPE, LBA_VIO_PARAMS_DTYPE,
                                    NAVSTATE_DTYPE, SBP_RIG_DTYPE)
from vieo_slam_amd.orb_extractor import KEYPOINT_DTYPE

N = 6
# which point each key of a key frame holds when it is inserted (key frame 0 makes the points from its stereo depth)
DEPTH0 = [3, 1, 2, 5, 4, 0]        # nearest first: keys 1, 2, 0, 4, 3 -> points 0 .. 4; key 5 has no depth
REF = {1: [0, 1, -1, 0, 2, -1],    # keys 0 and 3 (cameras 0 and 1 of the rig) both see point 0
       2: [2, -1, 0, 3, -1, -1]}
TABLE = {  # point -> key frame -> keys, under the replace rule
    0: {0: (1,), 1: (3,), 2: (2,)}, 1: {0: (2,), 1: (1,)}, 2: {0: (0,), 1: (4,), 2: (0,)}, 3: {0: (4,), 2: (3,)}, 4: {0: (3,)}}


class FakeStages:
    def __init__(self):
        self.R, self.erase, self.calls, self.und = None, set(), [], []

    def scale_factors(self):
        return 1.2 ** np.arange(8)

    def _solve(self, name, params, kfs, pts, obs, imu):
        self.calls.append(dict(name=name, params=params.copy(), kfs=kfs.copy(), obs=obs.copy(), imu=imu))
        erase = np.array([(int(o["kf"]), int(o["mp"])) in self.erase for o in obs], np.uint8)
        return kfs["nav"].copy(), pts.copy(), erase, np.zeros(1, LBA_RESULT_DTYPE)[0]

    def lba_vio(self, params, kfs, pts, close, obs, imu):
        return self._solve("lba_vio", params, kfs, pts, obs, imu)

    def lba(self, params, kfs, pts, obs):
        return self._solve("lba", params, kfs, pts, obs, None)

    def update_normal_depth(self, points, first, obs_centre, centres, ref_centre, ref_scale, scale_last):
        ids = [int(np.nonzero((self.R.mp_X == p).all(1))[0][0]) for p in points]
        self.und.append((ids, first.tolist(), obs_centre.tolist(), ref_centre.tolist()))
        return self.R.mp_normal[ids], self.R.mp_maxd[ids], self.R.mp_mind[ids]


def _frame(kid, mp_ref=None):
    f = replay._Frame()
    f.k, f.t, f.N = 10 * kid, 100.0 + 0.5 * kid, N
    f.keys = np.zeros(N, KEYPOINT_DTYPE)
    f.keys["x"], f.keys["y"], f.keys["octave"] = 100 + 10 * np.arange(N) + kid, 50 + 5 * np.arange(N), np.arange(N) % 3
    f.desc = np.full((N, 32), 16 * kid, np.uint8) + np.arange(N, dtype=np.uint8)[:, None]
    f.uright = (f.keys["x"] - 2).astype(np.float32)
    f.depth = np.array(DEPTH0 if kid == 0 else [0] * N, np.float32)
    f.key_cam = (np.arange(N) // 3).astype(np.int32)
    f.mp_ref = np.full(N, -1, np.int64) if mp_ref is None else np.array(mp_ref, np.int64)
    f.track_depth = np.full(N, np.inf, np.float32)
    return f


def _build(mode):
    S = FakeStages()
    if mode == "vision":
        R = rm.VisionReplay(None, S)
    else:
        R = replay.Replay(None, S)
    if mode == "rig":  # the data replay_modes.RigReplay's constructor sets, on a two-camera table
        R.one_key_per_kf, R.th_depth, R.cams = False, 35.0, np.zeros(2, CAMERA_DTYPE)
        rig = np.zeros(1, SBP_RIG_DTYPE)
        rig[0]["n_cams"] = 2
        R._set_cameras(rig, replay.K, 40.0, 0.1, np.tile(replay.BOUNDS, (2, 1)))
    S.R = R
    for kid in range(3):
        nav = np.zeros(1, NAVSTATE_DTYPE)[0]
        nav["p"], nav["q"] = (0.1 * kid, 0, 0), synth_ba._R_to_quat(np.eye(3))
        edge = np.zeros(1, IMU_PREINT_DTYPE)[0] if kid and R.inertial else None
        R.insert_keyframe(_frame(kid, REF.get(kid)), nav, edge)
    return R, S


def _expected_table(mode):
    t = {m: dict(ob) for m, ob in TABLE.items()}
    if mode == "rig":
        t[0][1] = (0, 3)
    return [t[m] for m in range(5)]


def _check_rows(R, job, call, order, pts, mode):
    """rows / obs of a window against the table: points in first-seen order, key frames ascending, keys ascending"""
    index = {kid: i for i, kid in enumerate(order)}
    want = [(index[kid], j, kid, i) for j, m in enumerate(pts) for kid in sorted(R.mp_obs[m]) if kid in index
            for i in sorted(R.mp_obs[m][kid])]
    assert [(r[0] & 0xFFFFFF, r[1], r[6], r[7]) for r in job["rows"]] == want
    obs = call["obs"]
    assert len(obs) == len(want)
    for o, (ix, j, kid, i) in zip(obs, want):
        k = R.kfs[kid]
        assert int(o["kf"]) & 0xFFFFFF == ix and int(o["mp"]) == j
        assert int(o["kf"]) >> 24 == (int(k.key_cam[i]) if mode == "rig" else 0)
        assert (o["u"], o["v"]) == (k.keys["x"][i], k.keys["y"][i]) and o["inv_sigma2"] == R.inv_sigma2[k.keys["octave"][i]]
        assert o["ur"] == (-1.0 if mode == "rig" else k.uright[i])
    return want


@pytest.mark.parametrize("mode", ["vio", "rig", "vision"])
def test_replay_map_table_window_and_write_back(mode):
    R, S = _build(mode)
    inertial = mode != "vision"
    assert R.one_key_per_kf == (mode != "rig") and R.inertial == inertial
    # ---- insert_keyframe: the new points nearest first, every key's observation through _add_obs
    assert R.kfs[0].mp_ref.tolist() == [2, 0, 1, 4, 3, -1] and len(R.mp_X) == 5 and not R.mp_bad.any()
    assert np.array_equal(R.mp_desc, R.kfs[0].desc[[1, 2, 0, 4, 3]])
    assert R.mp_obs == _expected_table(mode)
    # ---- the window of the last two key frames
    R.n_local = 2
    job = R.local_ba(apply=False)
    call = S.calls[-1]
    assert call["name"] == ("lba_vio" if inertial else "lba")
    assert call["params"].dtype == (LBA_VIO_PARAMS_DTYPE if inertial else LBA_PARAMS_DTYPE)
    base = call["params"][0]["base"] if inertial else call["params"][0]
    assert (int(base["its0"]), int(base["its1"])) == ((4, 6) if inertial else (5, 10))
    assert int(base["n_cams"]) == (2 if mode == "rig" else 0) and bool(base["cams"]) == (mode == "rig")
    assert job["pts"] == [0, 1, 2, 3] and [k.id for k in job["local"]] == [1, 2]
    assert call["kfs"]["fixed"].tolist() == [0, 0, 1]  # key frame 0: before the window (inertial) / an observer (vision)
    want = _check_rows(R, job, call, [1, 2, 0], job["pts"], mode)
    keys_of = [(kid, i) for _, j, kid, i in want if j == 0]  # point 0: key frames ascending, the rig's two keys ascending
    assert keys_of == ([(0, 1), (1, 0), (1, 3), (2, 2)] if mode == "rig" else [(0, 1), (1, 3), (2, 2)])
    if inertial:  # one IMU edge per local key frame whose predecessor is in the window: (kf0 -> kf1), (kf1 -> kf2)
        assert [(int(e["kf_i"]), int(e["kf_j"])) for e in call["imu"]] == [(2, 0), (0, 1)]
    assert R.stats["lba_shapes"][-1] == (3, 1, 4, len(want))  # (key frames, fixed ones, points, observations)
    # ---- the window of the last key frame alone: which key frames are fixed, and in which order
    R.n_local = 1
    job = R.local_ba(apply=False)
    call = S.calls[-1]
    assert job["pts"] == [2, 0, 3]
    # inertial: the key frame before the window first, then the observers as the points name them; else the observers only
    order = [2, 1, 0] if inertial else [2, 0, 1]
    assert call["kfs"]["fixed"].tolist() == [0, 1, 1]
    assert [tuple(k["nav"]["p"]) for k in call["kfs"]] == [tuple(R.kfs[kid].nav["p"]) for kid in order]
    _check_rows(R, job, call, order, job["pts"], mode)
    # ---- the write-back over all three key frames: one key of point 0 in key frame 1 and point 4's only observation erased
    R.n_local = 3
    cam1 = (1 << 24) if mode == "rig" else 0
    S.erase = {(1, 1), (0 | cam1, 3)}  # (kf field, point index in the window): pts = [2, 0, 1, 4, 3]
    job = R.local_ba(apply=False)
    assert job["pts"] == [2, 0, 1, 4, 3] and S.calls[-1]["kfs"]["fixed"].tolist() == [1, 0, 0]
    _check_rows(R, job, S.calls[-1], [0, 1, 2], job["pts"], mode)
    assert int(job["erase"].sum()) == 2
    before = [k.mp_ref.copy() for k in R.kfs]
    normal, applied = R.mp_normal.copy(), R.stats["lba_applied"]
    R._lba_apply(job)
    assert R.stats["lba_applied"] == applied + 1
    table = _expected_table(mode)
    if mode == "rig":
        table[0][1], gone = (3,), (1, 0)   # the two-key list loses key 0 (camera 0), key 3 goes on observing
    else:
        del table[0][1]                    # the one key of key frame 1 (key 3: it replaced key 0) goes, and the key frame with it
        gone = (1, 3)
    table[4] = {}
    assert R.mp_obs == table
    assert R.mp_bad.tolist() == [False, False, False, False, True]
    for kid, k in enumerate(R.kfs):  # every touched entry is reset, no other one
        want_ref = before[kid].copy()
        for kk, i in (gone, (0, 3)):
            if kk == kid:
                want_ref[i] = -1
        assert k.mp_ref.tolist() == want_ref.tolist()
    # UpdateNormalAndDepth for the window's points that are left, observers ascending, the oldest one the reference
    ids, first, obs_centre, ref = S.und[-1]
    assert ids == [2, 0, 1, 3] and np.array_equal(R.mp_normal, normal)
    assert obs_centre == [kid for m in ids for kid in sorted(table[m])] and ref == [0, 0, 0, 0]
    assert first == np.concatenate([[0], np.cumsum([len(table[m]) for m in ids])]).tolist()
    # ---- a second _add_obs of one key frame: replaces under one rule, extends (sorted, no duplicate) under the other
    R._add_obs(3, 2, 5)
    R._add_obs(3, 2, 1)
    R._add_obs(3, 2, 5)
    assert R.mp_obs[3] == {0: (4,), 2: ((5,) if R.one_key_per_kf else (1, 3, 5))}
