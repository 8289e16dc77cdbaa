"""Loop verification on the device (reference LoopClosing::ComputeSim3, src/LoopClosing.cc:308-489).  SearchByBoWKF --
ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*) of the current key frame against all candidates in one call --, Sim3Solver
-- the reference's Sim3Solver for a batch of candidates (every RANSAC hypothesis of every candidate in one launch,
iterate / find / GetEstimated* as look-ups) -- with draw_samples and sim3_correspondences (the constructor on flat
key-frame arrays), SearchBySim3 -- ORBmatcher::SearchBySim3 for a list of (candidate, Sim3) visits in one call, on
LoopKeyFrame records --, OptimizeSim3, and make_sim3_scene / make_bow_kf_scene / make_loop_pair_scene, the generators of
the tests and of tools/time_loop_sim3.py.  Loop closing (LoopClosing.cc:466, :682-707): SearchByProjectionScw --
ORBmatcher::SearchByProjection(KeyFrame*, Scw, ...) -- and FuseScw / SearchAndFuse -- ORBmatcher::Fuse(KeyFrame*, Scw,
...) of every corrected key frame in one call --, with make_loop_close_scene; ComputeSim3 -- the round-robin of
LoopClosing::ComputeSim3 as one call, then the final search and the nTotalMatches decision --, with
make_compute_sim3_scene.  The gather of the loop points, MapPoint::Replace and the map are not here."""
import ctypes

import numpy as np

from . import _lib
from .ba_types import CAMERA_DTYPE
from .map_point import FUSE_POINT_DTYPE
from .relocalization import BOW_KEYS_DTYPE, CAMERA_K, HEIGHT, WIDTH, BowKeys, _unpack_masks, rodrigues
from .relocalization import draw_samples as _draw_samples

SIM3_CANDIDATE_DTYPE = np.dtype([("n", np.int32), ("n1", np.int32), ("X1", np.uint64), ("X2", np.uint64),
                                 ("max_err1", np.uint64), ("max_err2", np.uint64), ("index1", np.uint64),
                                 ("cam1", np.uint64), ("cam2", np.uint64), ("cams1", np.uint64), ("cams2", np.uint64),
                                 ("n_cams1", np.int32), ("n_cams2", np.int32), ("fix_scale", np.int32),
                                 ("reserved", np.int32)], align=True)
SIM3_PARAMS_DTYPE = np.dtype([("probability", np.float64), ("min_inliers", np.int32), ("max_iterations", np.int32)],
                             align=True)
SIM3_INFO_DTYPE = np.dtype([("n", np.int32), ("n1", np.int32), ("min_inliers", np.int32), ("max_its", np.int32),
                            ("n_rows", np.int32), ("mask_words", np.int32), ("iterations", np.int32),
                            ("best_inliers", np.int32), ("best_row", np.int32), ("reserved", np.int32)], align=True)

# LoopClosing.cc:356: pSolver->SetRansacParameters(0.99, minInliers, 300), minInliers = thresh_inliers_ (20)
LOOP_SIM3_PARAMS = dict(probability=0.99, min_inliers=20, max_iterations=300)


def draw_samples(rng, n, n_rows):
    """n_rows minimal sets of 3 indices < n, each drawn without replacement the way Sim3Solver::iterate does
    (Sim3Solver.cc:164-178; relocalization.draw_samples with 3 per row)."""
    return _draw_samples(rng, n, n_rows, 3)


def max_error(sigma2):
    """mvnMaxError: the threshold 9.210 * sigma2 lands in a std::vector<size_t> (Sim3Solver.h:61-62), so it is the product
    taken in double from the float sigma2, truncated to an integer"""
    return (9.210 * np.asarray(sigma2, np.float32).astype(np.float64)).astype(np.int64).astype(np.int32)


def pinhole_camera(K=CAMERA_K):
    """the camera table of the rectified configuration (usedistort_ false): one pinhole, Tcr = identity"""
    c = np.zeros(1, CAMERA_DTYPE)
    c["fx"], c["fy"], c["cx"], c["cy"] = K
    c["Rcb"] = np.eye(3).reshape(-1)
    return c


def sim3_correspondences(mp_id1, matched12, index_in_kf2, Pw, Tcw1, Tcw2, octave1, octave2, level_sigma2_1, level_sigma2_2,
                         cam_of_key1=None, cam_of_key2=None, cams1=None, cams2=None, fix_scale=False):
    """Sim3Solver's constructor (Sim3Solver.cc:22-116) on flat key-frame arrays.
    mp_id1[N1]: GetMapPointMatches() of kf1 as ids (-1: NULL or isBad()); matched12[N1]: vpMatched12 as ids (-1: NULL or
    isBad()); index_in_kf2: id -> the key indices GetIndexInKeyFrame(pKF2) returns (several on a rig; negative ones
    are skipped); Pw: id -> GetWorldPos(); Tcw1 / Tcw2: 4 x 4; octave / level_sigma2: mvKeys[i].octave and
    scalepyrinfo_.vlevelsigma2_ of either side; cam_of_key: get<0>(mapn2in_[i]) per key (None: usedistort_ false, camera
    0); cams: CAMERA_DTYPE tables with Tcr in Rcb / tcb (None: one pinhole).  returns a candidate for Sim3Solver."""
    T1, T2 = np.asarray(Tcw1, np.float32), np.asarray(Tcw2, np.float32)
    lv1, lv2 = np.asarray(level_sigma2_1, np.float32), np.asarray(level_sigma2_2, np.float32)
    X1, X2, me1, me2, index1, cam1, cam2 = [], [], [], [], [], [], []
    for i1 in range(len(matched12)):
        mp2 = int(matched12[i1])
        if mp2 < 0:
            continue
        mp1 = int(mp_id1[i1])
        if mp1 < 0:
            continue
        for i2 in index_in_kf2[mp2]:
            if i2 < 0:
                continue
            me1.append(lv1[octave1[i1]])
            me2.append(lv2[octave2[i2]])
            index1.append(i1)
            X1.append(T1[:3, :3] @ np.asarray(Pw[mp1], np.float32) + T1[:3, 3])
            X2.append(T2[:3, :3] @ np.asarray(Pw[mp2], np.float32) + T2[:3, 3])
            cam1.append(0 if cam_of_key1 is None else int(cam_of_key1[i1]))
            cam2.append(0 if cam_of_key2 is None else int(cam_of_key2[i2]))
    n = len(index1)
    return dict(X1=np.array(X1, np.float32).reshape(n, 3), X2=np.array(X2, np.float32).reshape(n, 3),
                max_err1=max_error(np.array(me1, np.float32)), max_err2=max_error(np.array(me2, np.float32)),
                index1=np.array(index1, np.int32), n1=len(matched12), cam1=np.array(cam1, np.int32),
                cam2=np.array(cam2, np.int32), cams1=pinhole_camera() if cams1 is None else cams1,
                cams2=pinhole_camera() if cams2 is None else cams2, fix_scale=bool(fix_scale))


class _Candidate:
    def __init__(self, c):
        self.X1 = np.ascontiguousarray(c["X1"], np.float32).reshape(-1, 3)
        self.X2 = np.ascontiguousarray(c["X2"], np.float32).reshape(-1, 3)
        n = len(self.X1)
        self.max_err1 = np.ascontiguousarray(c["max_err1"], np.int32).reshape(-1)
        self.max_err2 = np.ascontiguousarray(c["max_err2"], np.int32).reshape(-1)
        self.index1 = np.ascontiguousarray(c["index1"], np.int32).reshape(-1)
        self.cam1 = np.ascontiguousarray(c.get("cam1", np.zeros(n)), np.int32).reshape(-1)
        self.cam2 = np.ascontiguousarray(c.get("cam2", np.zeros(n)), np.int32).reshape(-1)
        self.cams1 = np.ascontiguousarray(c.get("cams1", pinhole_camera()), CAMERA_DTYPE)
        self.cams2 = np.ascontiguousarray(c.get("cams2", pinhole_camera()), CAMERA_DTYPE)
        self.n1, self.fix_scale = int(c["n1"]), bool(c.get("fix_scale", False))
        if not all(len(a) == n for a in (self.X2, self.max_err1, self.max_err2, self.index1, self.cam1, self.cam2)):
            raise ValueError("Sim3Solver: the arrays of a candidate differ in length")

    def record(self):
        rec = np.zeros(1, SIM3_CANDIDATE_DTYPE)
        rec["n"], rec["n1"] = len(self.X1), self.n1
        for name in ("X1", "X2", "max_err1", "max_err2", "index1", "cam1", "cam2", "cams1", "cams2"):
            rec[name] = getattr(self, name).ctypes.data
        rec["n_cams1"], rec["n_cams2"], rec["fix_scale"] = len(self.cams1), len(self.cams2), int(self.fix_scale)
        return rec


def _params_record(params):
    p = dict(LOOP_SIM3_PARAMS)
    p.update(params or {})
    rec = np.zeros(1, SIM3_PARAMS_DTYPE)
    for k, v in p.items():
        rec[k] = v
    return rec


class Sim3Result:
    def __init__(self, found, T12, inliers, n_inliers, no_more, row):
        self.found, self.T12, self.inliers, self.n_inliers, self.no_more, self.row = found, T12, inliers, n_inliers, no_more, row


class Sim3Solver:
    """Sim3Solver of K loop candidates at once.

    candidates: a list of dicts with X1 (n, 3), X2 (n, 3), max_err1 (n,), max_err2 (n,) -- integers, see max_error --,
    index1 (n,), n1 and optionally cam1 / cam2 (n,), cams1 / cams2 (CAMERA_DTYPE tables, Tcr in Rcb / tcb) and fix_scale:
    what Sim3Solver's constructor collects (sim3_correspondences builds one).  samples: (K, S, 3) indices from
    draw_samples (a list of K arrays (S, 3) will do), or None to let the library draw from `seed`.  All hypotheses are
    evaluated when the object is made; iterate(c, n) is Sim3Solver::iterate of candidate c."""

    def __init__(self, candidates, samples=None, n_rows=None, seed=0, params=None):
        self._h = None
        self._cands = [_Candidate(c) for c in candidates]
        K = len(self._cands)
        if samples is not None:
            samples = np.ascontiguousarray(np.stack([np.asarray(s, np.int32).reshape(-1, 3) for s in samples]))
            n_rows = samples.shape[1]
        elif n_rows is None:
            raise ValueError("Sim3Solver: pass samples or n_rows")
        self.n_rows = int(n_rows)
        recs = np.concatenate([c.record() for c in self._cands]) if K else np.zeros(0, SIM3_CANDIDATE_DTYPE)
        par = _params_record(params)
        h = ctypes.c_void_p()
        rc = _lib.lib().vieo_sim3_create(ctypes.byref(h), recs.ctypes.data, K, par.ctypes.data,
                                         samples.ctypes.data if samples is not None else None, self.n_rows, int(seed))
        _lib.check(rc, "vieo_sim3_create")
        self._h = h

    def close(self):
        if self._h:
            _lib.lib().vieo_sim3_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self, c):
        rec = np.zeros(1, SIM3_INFO_DTYPE)
        _lib.check(_lib.lib().vieo_sim3_get_info(self._h, c, rec.ctypes.data), "vieo_sim3_get_info")
        return {k: int(rec[k][0]) for k in SIM3_INFO_DTYPE.names if k != "reserved"}

    def iterate_call(self, c, n_iterations):
        """vieo_sim3_iterate, raw: (rc, Sim3Result)"""
        cand = self._cands[c]
        found, n_inl, no_more, row = (ctypes.c_int32() for _ in range(4))
        T12 = np.zeros((4, 4), np.float32)
        inl = np.zeros(max(cand.n1, 1), np.uint8)
        rc = _lib.lib().vieo_sim3_iterate(self._h, c, int(n_iterations), ctypes.byref(found), T12.ctypes.data, inl.ctypes.data,
                                          ctypes.byref(n_inl), ctypes.byref(no_more), ctypes.byref(row))
        ok = bool(found.value)
        return rc, Sim3Result(ok, T12 if ok else None, inl[:cand.n1].astype(bool), n_inl.value, bool(no_more.value), row.value)

    def iterate(self, c, n_iterations):
        """cv::Mat Sim3Solver::iterate(nIterations, bNoMore, vbInliers, nInliers)"""
        rc, res = self.iterate_call(c, n_iterations)
        _lib.check(rc, "vieo_sim3_iterate")
        return res

    def find(self, c):
        """cv::Mat Sim3Solver::find(vbInliers12, nInliers): iterate(mRansacMaxIts)"""
        return self.iterate(c, self.info(c)["max_its"])

    def estimate(self, c):
        """GetEstimatedRotation / Translation / Scale: (R12 (3, 3), t12 (3,), s12) float32, or None before any iteration"""
        R, t, s = np.zeros((3, 3), np.float32), np.zeros(3, np.float32), ctypes.c_float()
        rc = _lib.lib().vieo_sim3_get_estimate(self._h, c, R.ctypes.data, t.ctypes.data, ctypes.byref(s))
        if rc == _lib.VIEO_E_EMPTY:
            return None
        _lib.check(rc, "vieo_sim3_get_estimate")
        return R, t, np.float32(s.value)

    def rows(self, c):
        """test tap: samples (S, 3), sRt (S, 13) = R row-major, t, s, count (S,), mask (S, n) bool"""
        i, S = self.info(c), self.n_rows
        smp, sRt, cnt = np.zeros((S, 3), np.int32), np.zeros((S, 13)), np.zeros(S, np.int32)
        words = np.zeros((S, max(i["mask_words"], 1)), np.uint64)
        _lib.check(_lib.lib().vieo_sim3_tap_rows(self._h, c, smp.ctypes.data, sRt.ctypes.data, cnt.ctypes.data,
                                                 words.ctypes.data), "vieo_sim3_tap_rows")
        return smp, sRt, cnt, _unpack_masks(words, i["n"])


def SearchByBoWKF(kf1, kf2s, mfNNratio=0.75, mbCheckOrientation=True):
    """int ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) of the key frame kf1 against every key frame of the list, in
    one call (BowKeys with mp_id on both sides).  returns [(match12 int32[kf1.N] -- the key of the candidate whose map
    point vpMatches12[i1] holds, -1 none --, the reference's return value)] per candidate."""
    recs = np.concatenate([k.rec for k in kf2s])
    n = len(kf1.keys)
    match = np.full((len(kf2s), max(n, 1)), -1, np.int32)
    n_matches = np.zeros(len(kf2s), np.int32)
    rc = _lib.lib().vieo_search_by_bow_kf(kf1.rec.ctypes.data, recs.ctypes.data, len(kf2s), float(mfNNratio),
                                          int(bool(mbCheckOrientation)), match.ctypes.data, n_matches.ctypes.data)
    _lib.check(rc, "vieo_search_by_bow_kf")
    return [(match[p, :n].copy(), int(n_matches[p])) for p in range(len(kf2s))]


# ---------------------------------------------------------------------------------------------------------------------
# scenes
def _rig(n_cams):
    """(cams with Tcr in Rcb / tcb, image size, [Trc 4 x 4]): one rectified pinhole, the 2-camera Radtan rig or the
    4-camera KB8 rig of synth_ba.camera_rig"""
    if n_cams == 1:
        return pinhole_camera(), (WIDTH, HEIGHT), [np.eye(4)]
    from .synth_ba import camera_rig
    cams, size, Tcr = camera_rig({2: "radtan", 4: "kb8"}[n_cams], with_tcr=True)
    cams = cams.copy()
    for i, T in enumerate(Tcr):
        cams[i]["Rcb"], cams[i]["tcb"] = T[:3, :3].reshape(-1), T[:3, 3]
    return cams, size, [np.linalg.inv(T) for T in Tcr]


def make_sim3_scene(seed, n=60, outlier_share=0.2, noise=0.01, fix_scale=False, n_cams=1, rng=None):
    """One candidate's correspondences: map points at 4-12 m in front of a camera of key frame 1's rig (n_cams = 1: the
    rectified 752 x 480 pinhole; 2: the Radtan rig; 4: the KB8 rig), the same points in the candidate's rig frame through
    the true S12 (rotation vector ~ N(0, 0.1 rad) per axis, translation ~ N(0, 0.3 m), scale 1 or uniform in
    [0.8, 1.25]), Gaussian noise of `noise` metres on both sides, outlier_share of the candidate's points replaced by
    others in view.  Keys on octaves 0..3 with sigma2 = 1.2^(2 octave); on a rig every fourth point is seen by a second
    camera of the candidate, which gives a second correspondence with the same index1.  n counts correspondences.
    Points are rounded to float32 like mvX3Dc1 / mvX3Dc2."""
    rng = np.random.default_rng(seed) if rng is None else rng
    cams, (W, H), Trc = _rig(n_cams)
    R12, t12 = rodrigues(rng.standard_normal(3) * 0.1), rng.standard_normal(3) * 0.3
    s12 = 1.0 if fix_scale else float(rng.uniform(0.8, 1.25))
    n_pts = n if n_cams == 1 else n - n // 5
    f = float(cams[0]["fx"])

    def in_view(k, cam):
        u, v, z = rng.uniform(0.2 * W, 0.8 * W, k), rng.uniform(0.2 * H, 0.8 * H, k), rng.uniform(4.0, 12.0, k)
        Pc = np.stack([(u - W / 2) / f * z, (v - H / 2) / f * z, z], axis=1)
        return np.stack([Trc[c][:3, :3] @ p + Trc[c][:3, 3] for c, p in zip(cam, Pc)])

    cam1 = rng.integers(0, n_cams, n_pts)
    X1 = in_view(n_pts, cam1)
    X2 = (X1 - t12) @ R12 / s12  # S12^-1
    n_out = int(round(n_pts * outlier_share))
    bad = rng.choice(n_pts, n_out, replace=False)
    X2[bad] = in_view(n_out, cam1[bad])
    truth = np.ones(n_pts, bool)
    truth[bad] = False
    X1, X2 = X1 + rng.standard_normal((n_pts, 3)) * noise, X2 + rng.standard_normal((n_pts, 3)) * noise
    octave1, octave2 = rng.integers(0, 4, n_pts), rng.integers(0, 4, n_pts)
    n1 = n_pts + 7
    index1 = np.sort(rng.choice(n1, n_pts, replace=False))
    cam2 = cam1.copy()
    order = np.arange(n_pts)
    if n_cams > 1:  # a second view in the candidate: the correspondence is repeated with another camera of its rig
        twice = np.sort(rng.choice(n_pts, n - n_pts, replace=False))
        order = np.sort(np.concatenate([order, twice]), kind="stable")
        second = np.zeros(len(order), bool)
        second[1:] = order[1:] == order[:-1]
        cam2 = np.where(second, (cam1[order] + 1) % n_cams, cam1[order])
    pick = lambda a: np.ascontiguousarray(np.asarray(a)[order])
    sigma2 = (np.float32(1.2) ** np.arange(8)).astype(np.float32) ** 2
    return dict(R12=R12, t12=t12, s12=s12, X1=pick(X1).astype(np.float32), X2=pick(X2).astype(np.float32),
                max_err1=max_error(sigma2[pick(octave1)]), max_err2=max_error(sigma2[pick(octave2)]),
                index1=pick(index1).astype(np.int32), n1=n1, cam1=pick(cam1).astype(np.int32),
                cam2=(cam2 if n_cams > 1 else pick(cam2)).astype(np.int32), cams1=cams, cams2=cams.copy(),
                fix_scale=bool(fix_scale), truth=pick(truth))


def make_bow_kf_scene(seed, n_cands=3, n_keys=300, n_nodes=40):
    """The current key frame and n_cands loop candidates for SearchByBoW(KF, KF): n_keys keys each in about n_nodes
    vocabulary nodes, three quarters of the keys of either side with a map point.  About 60 % of a candidate's keys are
    views of keys of the current key frame (a few descriptor bits flipped, the same node, its angle plus the candidate's
    rotation); planted on top: current keys with a near-duplicate in their node (the ratio test rejects), candidate keys
    that copy another one's descriptor (taken when their turn comes: vbMatched2), map points held by two keys of the
    current key frame (the (map point, 0) table replaces or keeps), views with a random angle (the rotation histogram
    removes them).  The last candidate lies in vocabulary nodes of its own: no node is shared.
    returns (BowKeys current, [BowKeys candidates])."""
    from .orb_extractor import KEYPOINT_DTYPE
    rng = np.random.default_rng(seed)
    node_ids = np.sort(rng.choice(100000, n_nodes + 4 * n_cands + 12, replace=False)).astype(np.uint32)
    shared, rest = node_ids[:n_nodes], node_ids[n_nodes:]

    def flip(desc, nbits):
        d = desc.copy()
        for b in rng.choice(256, nbits, replace=False):
            d[b // 8] ^= np.uint8(1 << (b % 8))
        return d

    def keys_of(angles):
        k = np.zeros(len(angles), KEYPOINT_DTYPE)
        k["x"], k["y"] = rng.uniform(20, WIDTH - 20, len(angles)), rng.uniform(20, HEIGHT - 20, len(angles))
        k["size"], k["angle"], k["octave"] = 31.0, angles, rng.integers(0, 4, len(angles))
        return k

    def feat_vec(node_of):
        return [(int(n), [int(i) for i in np.flatnonzero(node_of == n)]) for n in np.unique(node_of)]

    c_desc = rng.integers(0, 256, (n_keys, 32), dtype=np.uint8)
    c_node = shared[rng.integers(0, n_nodes, n_keys)]
    c_angle = rng.uniform(0, 360, n_keys).astype(np.float32)
    c_mp = np.where(rng.uniform(size=n_keys) < 0.75, np.arange(n_keys), -1).astype(np.int32)
    for i in range(0, n_keys // 10):  # near-duplicates inside the current key frame: key 2i+1 repeats key 2i
        c_desc[2 * i + 1], c_node[2 * i + 1] = flip(c_desc[2 * i], 3), c_node[2 * i]
    pairs = rng.permutation(np.arange(n_keys // 5, n_keys))[:80].reshape(-1, 2)
    for a, b in pairs:  # a rig's map point: two keys of the current key frame hold it
        if c_mp[a] >= 0:
            c_mp[b] = c_mp[a]
    current = BowKeys(keys_of(c_angle), c_desc, feat_vec(c_node), c_mp)
    cands = []
    for p in range(n_cands):
        rot = rng.uniform(0, 360)
        k_desc = rng.integers(0, 256, (n_keys, 32), dtype=np.uint8)
        if p == n_cands - 1:
            own = rest[4 * p:4 * p + 12]
        else:
            own = np.concatenate([shared[p::2], rest[4 * p:4 * p + 4]])  # half the shared nodes + nodes of its own
        k_node = own[rng.integers(0, len(own), n_keys)]
        k_angle = rng.uniform(0, 360, n_keys).astype(np.float32)
        mp = np.where(rng.uniform(size=n_keys) < 0.75, np.arange(n_keys) + 1000 * (p + 1), -1).astype(np.int32)
        if p < n_cands - 1:
            views = rng.choice(n_keys, int(0.6 * n_keys), replace=False)
            src = rng.choice(n_keys, len(views), replace=False)
            for j, (a, b) in enumerate(zip(views, src)):
                k_desc[a], k_node[a] = flip(c_desc[b], int(rng.integers(0, 40))), c_node[b]
                ang = c_angle[b] - rot + rng.normal(0, 2.0) if j % 8 else rng.uniform(0, 360)
                k_angle[a] = np.float32(ang % 360.0)
            for j in range(0, 40, 2):  # a second candidate key that looks the same, with another map point
                a, b = views[j], views[j + 1]
                k_desc[b], k_node[b], k_angle[b] = flip(k_desc[a], 2), k_node[a], k_angle[a]
        k_angle[k_angle >= 360.0] = 0.0
        cands.append(BowKeys(keys_of(k_angle), k_desc, feat_vec(k_node), mp))
    return current, cands


# ---------------------------------------------------------------------------------------------------------------------
# SearchBySim3
LOOP_KEYFRAME_DTYPE = np.dtype([("bow", BOW_KEYS_DTYPE), ("cam_of_key", np.uint64), ("points", np.uint64),
                                ("cams", np.uint64), ("Rcw", "<f4", 9), ("tcw", "<f4", 3), ("Ow", "<f4", 3),
                                ("n_cams", "<i4"), ("use_distort", "<i4"), ("Tcr", "<f4", (4, 12)), ("trc", "<f4", (4, 3)),
                                ("bounds", "<f4", (4, 4)), ("scale_factors", "<f4", 16), ("level_sigma2", "<f4", 16),
                                ("inv_level_sigma2", "<f4", 16), ("log_scale_factor", "<f4"), ("n_levels", "<i4")],
                               align=True)
SIM3_VISIT_DTYPE = np.dtype([("kf2", "<i4"), ("s12", "<f4"), ("R12", "<f4", 9), ("t12", "<f4", 3), ("match12", np.uint64),
                             ("n_found", "<i4"), ("reserved", "<i4")], align=True)
assert LOOP_KEYFRAME_DTYPE.itemsize == 656 and SIM3_VISIT_DTYPE.itemsize == 72

TH_SIM3 = 7.5  # LoopClosing.cc:412: matcher.SearchBySim3(mpCurrentKF, pKF, vpMapPointMatches, s, R, t, 7.5)


def pyramid_tables(n_levels=8, scale_factor=1.2):
    """scalepyrinfo_ as ORBextractor fills it (ORBextractor.cc:417-432), in float: vscalefactor_, vlevelsigma2_,
    vinvlevelsigma2_, flogscalefactor_"""
    sc = np.ones(n_levels, np.float32)
    for i in range(1, n_levels):
        sc[i] = sc[i - 1] * np.float32(scale_factor)
    sigma2 = sc * sc
    return sc, sigma2, np.float32(1.0) / sigma2, np.float32(np.log(np.float32(scale_factor)))


class LoopKeyFrame:
    """A key frame as loop verification reads it, and its vieo_loop_keyframe record (arrays kept alive here).
    bow: BowKeys with mp_id; points: FUSE_POINT_DTYPE[n_keys], the map point of every key (read where mp_id >= 0);
    Tcw: 4 x 4 GetPose(); cam_of_key: get<0>(mapn2in_[i]) (None: camera 0); cams: CAMERA_DTYPE table (None: the rectified
    pinhole); Tcr: [4 x 4] per camera (None: identity); size: (width, height) of the undistorted image bounds;
    use_distort: usedistort_ (None: True on a rig)."""

    def __init__(self, bow, points, Tcw, cam_of_key=None, cams=None, Tcr=None, size=(WIDTH, HEIGHT), use_distort=None,
                 n_levels=8, scale_factor=1.2):
        self.bow, n = bow, len(bow.keys)
        self.keys, self.desc, self.mp_id = bow.keys, bow.desc, bow.mp_id
        self.points = np.ascontiguousarray(points, FUSE_POINT_DTYPE)
        self.cam_of_key = np.zeros(n, np.int32) if cam_of_key is None else np.ascontiguousarray(cam_of_key, np.int32)
        self.cams = np.ascontiguousarray(pinhole_camera() if cams is None else cams, CAMERA_DTYPE)
        self.n_cams = len(self.cams)
        self.use_distort = int(self.n_cams > 1 if use_distort is None else use_distort)
        T = np.asarray(Tcw, np.float32)
        self.Rcw, self.tcw = np.ascontiguousarray(T[:3, :3]), np.ascontiguousarray(T[:3, 3])
        self.Ow = -(self.Rcw.T @ self.tcw)  # KeyFrame::SetPose: Ow = -Rwc * tcw in float
        Tcr = [np.eye(4)] * self.n_cams if Tcr is None else Tcr
        self.Tcr = np.stack([np.asarray(t, np.float64)[:3, :].reshape(-1) for t in Tcr]).astype(np.float32)
        self.trc = np.stack([np.linalg.inv(np.asarray(t, np.float64))[:3, 3] for t in Tcr]).astype(np.float32)
        self.bounds = np.tile(np.array([0, size[0], 0, size[1]], np.float32), (self.n_cams, 1))
        self.n_levels = int(n_levels)
        self.scale_factors, self.level_sigma2, self.inv_level_sigma2, self.log_scale_factor = pyramid_tables(n_levels,
                                                                                                              scale_factor)
        r = np.zeros(1, LOOP_KEYFRAME_DTYPE)
        r["bow"] = bow.rec[0]
        r["cam_of_key"], r["points"], r["cams"] = self.cam_of_key.ctypes.data, self.points.ctypes.data, self.cams.ctypes.data
        r["Rcw"], r["tcw"], r["Ow"] = self.Rcw.reshape(-1), self.tcw, self.Ow
        r["n_cams"], r["use_distort"], r["n_levels"] = self.n_cams, self.use_distort, self.n_levels
        r["Tcr"][0, :self.n_cams], r["trc"][0, :self.n_cams], r["bounds"][0, :self.n_cams] = self.Tcr, self.trc, self.bounds
        for name in ("scale_factors", "level_sigma2", "inv_level_sigma2"):
            r[name][0, :n_levels] = getattr(self, name)
        r["log_scale_factor"] = self.log_scale_factor
        self.rec = r


def search_by_sim3_call(kf1, kf2s, visits, th=TH_SIM3):
    """vieo_search_by_sim3, raw: visits = [(candidate, s12, R12 (3, 3), t12 (3,), match12 int32[kf1.N])];
    returns (rc, [(match12 after the call, nFound)])"""
    recs = np.concatenate([k.rec for k in kf2s]) if kf2s else np.zeros(0, LOOP_KEYFRAME_DTYPE)
    V = np.zeros(len(visits), SIM3_VISIT_DTYPE)
    out = []
    for v, (c, s12, R12, t12, match12) in enumerate(visits):
        m = np.array(match12, np.int32).reshape(-1)
        out.append(m)
        V[v]["kf2"], V[v]["s12"] = c, s12
        V[v]["R12"], V[v]["t12"] = np.asarray(R12, np.float32).reshape(-1), np.asarray(t12, np.float32)
        V[v]["match12"] = m.ctypes.data
    rc = _lib.lib().vieo_search_by_sim3(kf1.rec.ctypes.data, recs.ctypes.data if len(recs) else None, len(kf2s),
                                        V.ctypes.data if len(V) else None, len(V), float(th))
    return rc, [(m, int(V[v]["n_found"])) for v, m in enumerate(out)]


def SearchBySim3(kf1, kf2s, visits, th=TH_SIM3):
    """int ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) for every visit of the list in one call.
    kf1, kf2s: LoopKeyFrame; visits: [(candidate index, s12, R12, t12, match12)] with match12[i1] the candidate's key
    whose map point vpMatches12[i1] holds (-1: NULL).  returns [(match12 after the call, the return value)]."""
    rc, out = search_by_sim3_call(kf1, kf2s, visits, th)
    _lib.check(rc, "vieo_search_by_sim3")
    return out


def search_by_sim3_tap(kf1, kf2, visit, direction):
    """the device stage of the last SearchBySim3: (best_idx, best_dist) int32[n_points, n_cams] of a visit, direction 0
    (kf1's points into the candidate kf2) or 1 (back); best_idx is a key of the target key frame"""
    src = kf1 if direction == 0 else kf2
    bi = np.zeros((max(len(src.keys), 1), src.n_cams), np.int32)
    bd = np.zeros_like(bi)
    _lib.check(_lib.lib().vieo_search_by_sim3_tap(visit, direction, bi.ctypes.data, bd.ctypes.data),
               "vieo_search_by_sim3_tap")
    return bi[:len(src.keys)], bd[:len(src.keys)]


# ---------------------------------------------------------------------------------------------------------------------
# OptimizeSim3
SIM3_OPT_VISIT_DTYPE = np.dtype([("kf2", "<i4"), ("reserved", "<i4"), ("s12", "<f8"), ("R12", "<f8", 9), ("t12", "<f8", 3),
                                 ("match12", np.uint64), ("n_inliers", "<i4"), ("n_correspondences", "<i4"), ("n_bad", "<i4"),
                                 ("iterations", "<i4", 2), ("trials", "<i4", 2), ("reserved2", "<i4")], align=True)
assert SIM3_OPT_VISIT_DTYPE.itemsize == 152
SIM3_OPT_MAX_TRIALS = 150
TH2_SIM3 = 10.0  # LoopClosing.cc:411: Optimizer::OptimizeSim3(mpCurrentKF, pKF, vpMapPointMatches, gScm, 10, mbFixScale)


def optimize_sim3_call(kf1, kf2s, visits, th2=TH2_SIM3, fix_scale=False):
    """vieo_optimize_sim3, raw: visits = [(candidate, s12, R12 (3, 3), t12 (3,), match12 int32[kf1.N])]; returns
    (rc, [dict(match12, s12, R12, t12, n_inliers, n_correspondences, n_bad, iterations, trials) after the call])"""
    recs = np.concatenate([k.rec for k in kf2s]) if kf2s else np.zeros(0, LOOP_KEYFRAME_DTYPE)
    V = np.zeros(len(visits), SIM3_OPT_VISIT_DTYPE)
    ms = []
    for v, (c, s12, R12, t12, match12) in enumerate(visits):
        m = np.array(match12, np.int32).reshape(-1)
        ms.append(m)
        V[v]["kf2"], V[v]["s12"] = c, s12
        V[v]["R12"], V[v]["t12"] = np.asarray(R12, np.float64).reshape(-1), np.asarray(t12, np.float64)
        V[v]["match12"] = m.ctypes.data
    rc = _lib.lib().vieo_optimize_sim3(kf1.rec.ctypes.data, recs.ctypes.data if len(recs) else None, len(kf2s),
                                       V.ctypes.data if len(V) else None, len(V), float(th2), int(bool(fix_scale)))
    return rc, [dict(match12=m, s12=float(V[v]["s12"]), R12=V[v]["R12"].reshape(3, 3).copy(), t12=V[v]["t12"].copy(),
                     n_inliers=int(V[v]["n_inliers"]), n_correspondences=int(V[v]["n_correspondences"]),
                     n_bad=int(V[v]["n_bad"]), iterations=V[v]["iterations"].tolist(), trials=V[v]["trials"].tolist())
                for v, m in enumerate(ms)]


def OptimizeSim3(kf1, kf2s, visits, th2=TH2_SIM3, fix_scale=False):
    """int Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale) for every visit of the list in one
    launch.  visits: the tuples SearchBySim3 takes, [(candidate index, s12, R12, t12, match12)], S12 in double.
    returns [(match12 after the call (erased correspondences are -1), (s12, R12, t12) after the call, nInliers)]."""
    rc, out = optimize_sim3_call(kf1, kf2s, visits, th2, fix_scale)
    _lib.check(rc, "vieo_optimize_sim3")
    return [(o["match12"], (o["s12"], o["R12"], o["t12"]), o["n_inliers"]) for o in out]


def optimize_sim3_trace(visit):
    """the test tap of the last OptimizeSim3: dict(trials [n, 4] = (chi2 before, chi2 after, lambda, accepted), i1 [n_corr],
    chi2 [2, n_corr, 2] = (chi2_12, chi2_21) as read at the two checks)"""
    nt, nc = ctypes.c_int32(0), ctypes.c_int32(0)
    L = _lib.lib()
    _lib.check(L.vieo_optimize_sim3_trace(visit, ctypes.byref(nt), None, ctypes.byref(nc), None, None), "vieo_optimize_sim3_trace")
    trials, i1 = np.zeros((SIM3_OPT_MAX_TRIALS, 4)), np.zeros(max(nc.value, 1), np.int32)
    chi2 = np.zeros((2, max(nc.value, 1), 2))
    _lib.check(L.vieo_optimize_sim3_trace(visit, None, trials.ctypes.data, None, i1.ctypes.data, chi2.ctypes.data),
               "vieo_optimize_sim3_trace")
    return dict(trials=trials[:nt.value].copy(), i1=i1[:nc.value].copy(), chi2=chi2.reshape(-1)[:4 * nc.value].reshape(2, nc.value, 2).copy())


def _project_f64(cams, Tcr, Pcr, c):
    from .synth_ba import project_camera
    Pc = Tcr[c][:3, :3] @ Pcr + Tcr[c][:3, 3]
    if Pc[2] < 0.3:
        return None
    if len(cams) > 1 and np.hypot(Pc[0], Pc[1]) / Pc[2] > (0.9 if cams[c]["model"] == 1 else 2.0):
        return None
    if len(cams) == 1:
        return float(cams[0]["fx"]) * Pc[0] / Pc[2] + float(cams[0]["cx"]), float(cams[0]["fy"]) * Pc[1] / Pc[2] + float(cams[0]["cy"])
    return project_camera(cams[c], Pc)


def make_loop_pair_scene(seed, n_keys=200, n_points=120, n_cams=1, n_cands=1, rig="radtan", plant=False):
    """The current key frame and n_cands loop candidates that see the same n_points physical points, for SearchBySim3.
    The candidates' maps are the real world; the current key frame's map has drifted by a similarity (scale in
    [0.93, 1.07], 0.02 rad, 0.1 m), so the true S12 of candidate c is s12 = the drift's scale, R12 = R1 R2^T, t12 =
    s12 (t1 - R12 t2) with the real poses.  Every key frame: one key per (map point, camera that sees it) -- noisy
    projection, the point's descriptor with up to 20 bits flipped, the octave the point's size predicts at the key
    frame's distance --, filled up to n_keys with keys without a map point; on a rig (n_cams = 2: the first two cameras
    of synth_ba.camera_rig(rig), usedistort_ true) the keys are in random order, so cameras interleave and a map point
    seen by both cameras is held by a key in each.  ids: the current key frame's 0 ..., candidate c's 1000 (c + 1) + j for
    the same physical point j.
    plant (one camera): on candidate 0, (a) a current key whose octave is off by 3 (the forward search hits, the backward
    one cannot agree), (b) a candidate key without a map point that copies a current point's descriptor at its projection
    (the best key holds no map point while a worse one does), (c) candidate keys 0.1 % inside and outside the window of
    their point.
    returns dict(kf1, kf2s, sim3=[(s12, R12, t12)], pairs=[{i1: i2}] (keys of the same physical point in camera 0 ...),
    planted=dict)."""
    from .orb_extractor import KEYPOINT_DTYPE
    rng = np.random.default_rng(seed)
    if n_cams == 1:
        cams, (W, H), Tcr = pinhole_camera(), (WIDTH, HEIGHT), [np.eye(4)]
    else:
        from .synth_ba import camera_rig
        cams, (W, H), Tcr = camera_rig(rig, with_tcr=True, n_cams=n_cams)
    f = float(cams[0]["fx"])
    # physical points in front of the current key frame's reference camera, real poses close to each other
    u, v, z = rng.uniform(0.2 * W, 0.8 * W, n_points), rng.uniform(0.2 * H, 0.8 * H, n_points), rng.uniform(4.0, 12.0, n_points)
    X1 = np.stack([(u - W / 2) / f * z, (v - H / 2) / f * z, z], axis=1)
    R1, t1 = rodrigues(rng.standard_normal(3) * 0.3), rng.standard_normal(3)
    Pw = (X1 - t1) @ R1
    size = z * 1.2 ** rng.integers(0, 4, n_points)  # the distance at which the point fills level 0
    base = rng.integers(0, 256, (n_points, 32), dtype=np.uint8)
    sd, Rd, td = float(rng.uniform(0.93, 1.07)), rodrigues(rng.standard_normal(3) * 0.02), rng.standard_normal(3) * 0.1

    def flip(d, nbits):
        d = d.copy()
        for b in rng.choice(256, nbits, replace=False):
            d[b // 8] ^= np.uint8(1 << (b % 8))
        return d

    def key_frame(R, t, drift, id0, shuffle):
        """keys of the real pose (R, t); the stored map and pose go through `drift` (s, R, t) or stay real"""
        ds, dR, dt = drift
        O = -R.T @ t
        rows = []  # (x, y, octave, camera, point or -1)
        for j in range(n_points):
            d = np.linalg.norm(Pw[j] - O)
            lvl = int(np.clip(np.rint(np.log(size[j] / d) / np.log(1.2)), 0, 7))
            for c in range(len(cams)):
                uv = _project_f64(cams, Tcr, R @ Pw[j] + t, c)
                if uv is None or not (8 < uv[0] < W - 8 and 8 < uv[1] < H - 8):
                    continue
                s = 1.2 ** lvl
                rows.append((uv[0] + rng.normal(0, 0.5) * s, uv[1] + rng.normal(0, 0.5) * s, lvl, c, j))
        rows = rows[:n_keys - 20]
        while len(rows) < n_keys:
            rows.append((rng.uniform(0, W), rng.uniform(0, H), int(rng.integers(0, 8)), int(rng.integers(0, len(cams))), -1))
        order = rng.permutation(n_keys) if shuffle else np.arange(n_keys)
        rows = [rows[i] for i in order]
        keys = np.zeros(n_keys, KEYPOINT_DTYPE)
        keys["x"], keys["y"] = [r[0] for r in rows], [r[1] for r in rows]
        keys["octave"], keys["size"], keys["angle"] = [r[2] for r in rows], 31.0, rng.uniform(0, 359, n_keys)
        phys = np.array([r[4] for r in rows])
        mp_id = np.where(phys >= 0, id0 + phys, -1).astype(np.int32)
        desc = np.stack([flip(base[j], int(rng.integers(0, 20))) if j >= 0 else rng.integers(0, 256, 32, dtype=np.uint8)
                         for j in phys])
        pts = np.zeros(n_keys, FUSE_POINT_DTYPE)
        Rm, tm = R @ dR.T, ds * t - R @ dR.T @ dt
        Om = -Rm.T @ tm
        mp_desc = {j: flip(base[j], 4) for j in set(phys[phys >= 0].tolist())}
        for i, j in enumerate(phys):
            if j < 0:
                continue
            Xm = ds * dR @ Pw[j] + dt
            dm = np.linalg.norm(Xm - Om)
            pts[i]["Xw"], pts[i]["normal"] = Xm, (Xm - Om) / dm
            pts[i]["max_distance"] = dm * 1.2 ** int(keys["octave"][i])
            pts[i]["min_distance"] = pts[i]["max_distance"] / np.float32(1.2 ** 7)
            pts[i]["desc"] = mp_desc[j]
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = Rm, tm
        return dict(keys=keys, desc=desc, mp_id=mp_id, pts=pts, T=T, cam=np.array([r[3] for r in rows], np.int32), phys=phys)

    shuffle = n_cams > 1
    k1 = key_frame(R1, t1, (sd, Rd, td), 0, shuffle)
    k2s, sim3, pairs = [], [], []
    for c in range(n_cands):
        R2, t2 = rodrigues(rng.standard_normal(3) * 0.05) @ R1, t1 + rng.standard_normal(3) * 0.3
        k2s.append(key_frame(R2, t2, (1.0, np.eye(3), np.zeros(3)), 1000 * (c + 1), shuffle))
        R12 = R1 @ R2.T
        sim3.append((np.float32(sd), R12.astype(np.float32), (sd * (t1 - R12 @ t2)).astype(np.float32)))
        first2 = {}
        for i2, (j, cm) in enumerate(zip(k2s[c]["phys"], k2s[c]["cam"])):
            if j >= 0:
                first2.setdefault((int(j), int(cm)), i2)
        pairs.append({i1: first2[(int(j), int(cm))] for i1, (j, cm) in enumerate(zip(k1["phys"], k1["cam"]))
                      if j >= 0 and (int(j), int(cm)) in first2})
    planted = {}
    if plant:
        assert n_cams == 1
        k2, (s12, R12, t12) = k2s[0], sim3[0]
        both = sorted(pairs[0].items())
        free2 = [int(i) for i in np.flatnonzero(k2["mp_id"] < 0)]
        (a1, _), (b1, b2), (in1, in2), (out1, out2) = both[3], both[7], both[11], both[15]
        k1["keys"]["octave"][a1] = min(int(k1["keys"]["octave"][a1]) + 3, 7)
        planted["no_backward"] = a1
        # the window of a current point in the candidate: its real projection, the level PredictScale gives there
        O2 = -k2["T"][:3, :3].T @ k2["T"][:3, 3]

        def window(i1):
            P = k1["pts"][i1]
            j = k1["phys"][i1]
            uv = _project_f64(cams, Tcr, k2["T"][:3, :3] @ Pw[j] + k2["T"][:3, 3], 0)
            d3 = np.linalg.norm(P["Xw"].astype(np.float64) - O2)
            lvl = int(np.clip(np.ceil(np.log(float(P["max_distance"]) / d3) / np.log(1.2)), 0, 7))
            return uv, lvl, TH_SIM3 * 1.2 ** lvl
        uv, lvl, _ = window(b1)
        d = free2[0]
        k2["keys"]["x"][d], k2["keys"]["y"][d], k2["keys"]["octave"][d] = uv[0], uv[1], lvl
        k2["desc"][d] = k1["pts"][b1]["desc"]
        planted["best_without_point"] = (b1, d, b2)
        for name, i1, i2, fac in (("edge_in", in1, in2, 0.999), ("edge_out", out1, out2, -1.001)):
            uv, lvl, radius = window(i1)
            k2["keys"]["x"][i2], k2["keys"]["y"][i2], k2["keys"]["octave"][i2] = uv[0] + fac * radius, uv[1], lvl
            planted[name] = (i1, i2)

    def loop_kf(k):
        bow = BowKeys(k["keys"], k["desc"], [], k["mp_id"])
        return LoopKeyFrame(bow, k["pts"], k["T"], k["cam"], cams, Tcr, (W, H))
    return dict(kf1=loop_kf(k1), kf2s=[loop_kf(k) for k in k2s], sim3=sim3, pairs=pairs, planted=planted)


def make_loop_optimize_scene(seed, n_pairs, n_outliers=0, n_cams=1, rig="radtan", perturb=1.0):
    """A visit for OptimizeSim3 on top of make_loop_pair_scene: the first n_pairs true pairs of candidate 0 become match12,
    the true S12 is turned by 0.4 perturb degrees, moved by 3 perturb cm and scaled by 1 + perturb %, and n_outliers of the
    pairs are planted as outliers by swapping the candidate keys of neighbouring pairs (a current map point then faces
    another physical point).  returns dict(kf1, kf2s, visit = (0, s12, R12, t12, match12), truth = (s12, R12, t12),
    outliers = the swapped keys of kf1)."""
    n_points = max(120, 2 * n_pairs)
    s = make_loop_pair_scene(seed, n_keys=n_points + 80, n_points=n_points, n_cams=n_cams, rig=rig)
    pairs = sorted(s["pairs"][0].items())
    assert len(pairs) >= n_pairs, (len(pairs), n_pairs)
    pairs = pairs[:n_pairs]
    match12 = np.full(len(s["kf1"].keys), -1, np.int32)
    for i1, i2 in pairs:
        match12[i1] = i2
    outliers = []
    for k in range(n_outliers // 2 + n_outliers % 2):  # swap pairs (4k, 4k + 2); an odd count takes one side of the last swap
        (a1, a2), (b1, b2) = pairs[4 * k], pairs[4 * k + 2]
        match12[a1] = b2
        outliers.append(a1)
        if len(outliers) < n_outliers:
            match12[b1] = a2
            outliers.append(b1)
    s12, R12, t12 = (np.asarray(a, np.float64) for a in s["sim3"][0])
    axis = np.array([0.004, -0.005, 0.003]) / np.linalg.norm([0.004, -0.005, 0.003])
    w = axis * np.deg2rad(0.4 * perturb)
    start = (float(s12) * (1 + 0.01 * perturb), rodrigues(w) @ R12, t12 + 0.03 * perturb)
    return dict(kf1=s["kf1"], kf2s=s["kf2s"], visit=(0,) + start + (match12,), truth=(float(s12), R12, t12), outliers=outliers)


# ---------------------------------------------------------------------------------------------------------------------
# the two projection searches through a Sim3 world pose Scw
SCW_VISIT_DTYPE = np.dtype([("kf", "<i4"), ("Scw", "<f4", 12), ("matched", np.uint64), ("n_matches", "<i4")], align=True)
FUSE_SCW_VISIT_DTYPE = np.dtype([("kf", "<i4"), ("Scw", "<f4", 12), ("match_key", np.uint64), ("replace", np.uint64),
                                 ("added", np.uint64), ("n_fused", "<i4"), ("reserved", "<i4")], align=True)
assert SCW_VISIT_DTYPE.itemsize == 72 and FUSE_SCW_VISIT_DTYPE.itemsize == 88
TH_SCW_SEARCH = 10.0  # LoopClosing.cc:466: matcher.SearchByProjection(mpCurrentKF, mScw, mvpLoopMapPoints, mvpCurrentMatchedPoints, 10)
TH_SCW_FUSE = 4.0     # LoopClosing.cc:697: matcher.Fuse(pKF, cvScw, mvpLoopMapPoints, 4, vpReplacePoints)
LOOP_MATCHES = 40     # LoopClosing.cc:475: nTotalMatches >= 40


def _point_table(points, ids):
    pts = np.ascontiguousarray(points, FUSE_POINT_DTYPE)
    ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
    if len(pts) != len(ids):
        raise ValueError("the point table and its ids differ in length")
    return pts, ids


def search_by_projection_scw_call(kfs, points, ids, visits, th=TH_SCW_SEARCH):
    """vieo_search_by_projection_scw, raw: visits = [(key frame index, Scw (3, 4), matched int32[n_keys])];
    returns (rc, [(matched after the call, nmatches)])"""
    recs = np.concatenate([k.rec for k in kfs]) if kfs else np.zeros(0, LOOP_KEYFRAME_DTYPE)
    pts, ids = _point_table(points, ids)
    V = np.zeros(len(visits), SCW_VISIT_DTYPE)
    out = []
    for v, (kf, Scw, matched) in enumerate(visits):
        m = np.array(matched, np.int32).reshape(-1)
        out.append(m)
        V[v]["kf"], V[v]["Scw"], V[v]["matched"] = kf, np.asarray(Scw, np.float32).reshape(-1), m.ctypes.data
        V[v]["n_matches"] = -7  # (a refused call leaves it)
    rc = _lib.lib().vieo_search_by_projection_scw(recs.ctypes.data if len(recs) else None, len(kfs),
                                                  pts.ctypes.data if len(pts) else None, ids.ctypes.data if len(ids) else None,
                                                  len(pts), V.ctypes.data if len(V) else None, len(V), float(th))
    return rc, [(m, int(V[v]["n_matches"])) for v, m in enumerate(out)]


def SearchByProjectionScw(kfs, points, ids, visits, th=TH_SCW_SEARCH):
    """int ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) for every visit of the list in one call.
    kfs: LoopKeyFrame list; points / ids: the loop map points (FUSE_POINT_DTYPE, bit 31 of skip_mask = isBad()) and their
    ids in the id space of mp_id; visits: [(key frame index, Scw 3 x 4 float = s R | t, matched)] with matched[i] the id
    vpMatched[i] holds (-1: NULL).  The visits are independent of one another: each starts from its own matched as given.
    returns [(matched after the call, the return value)]."""
    rc, out = search_by_projection_scw_call(kfs, points, ids, visits, th)
    _lib.check(rc, "vieo_search_by_projection_scw")
    return out


def search_by_projection_scw_tap(n_points, n_cams, visit):
    """the device stage of the last SearchByProjectionScw: [[(key, distance, position in the reference's candidate order)]
    per camera] per point -- every window key with distance <= TH_LOW, in candidate order"""
    L = _lib.lib()
    cnt = np.zeros((max(n_points, 1), n_cams), np.int32)
    _lib.check(L.vieo_search_by_projection_scw_tap(visit, cnt.ctypes.data, None, None, None, 0), "vieo_search_by_projection_scw_tap")
    cap = max(int(cnt.max()), 1)
    key, dist, order = (np.zeros(cnt.shape + (cap,), np.int32) for _ in range(3))
    _lib.check(L.vieo_search_by_projection_scw_tap(visit, None, key.ctypes.data, dist.ctypes.data, order.ctypes.data, cap),
               "vieo_search_by_projection_scw_tap")
    return [[[(int(key[m, c, e]), int(dist[m, c, e]), int(order[m, c, e])) for e in range(cnt[m, c])] for c in range(n_cams)]
            for m in range(n_points)]


def fuse_scw_call(kfs, points, ids, visits, th=TH_SCW_FUSE):
    """vieo_fuse_scw, raw: visits = [(key frame index, Scw (3, 4))]; returns (rc, [dict(match_key [n_points, n_cams],
    replace [n_points], added [n_points, n_cams], n_fused)])"""
    recs = np.concatenate([k.rec for k in kfs]) if kfs else np.zeros(0, LOOP_KEYFRAME_DTYPE)
    pts, ids = _point_table(points, ids)
    nc = kfs[0].n_cams if kfs else 1
    V = np.zeros(len(visits), FUSE_SCW_VISIT_DTYPE)
    out = []
    for v, (kf, Scw) in enumerate(visits):
        o = dict(match_key=np.full((max(len(pts), 1), nc), -7, np.int32), replace=np.full(max(len(pts), 1), -7, np.int32),
                 added=np.full((max(len(pts), 1), nc), 7, np.uint8))
        out.append(o)
        V[v]["kf"], V[v]["Scw"] = kf, np.asarray(Scw, np.float32).reshape(-1)
        for name in ("match_key", "replace", "added"):
            V[v][name] = o[name].ctypes.data
        V[v]["n_fused"] = -7
    rc = _lib.lib().vieo_fuse_scw(recs.ctypes.data if len(recs) else None, len(kfs), pts.ctypes.data if len(pts) else None,
                                  ids.ctypes.data if len(ids) else None, len(pts), V.ctypes.data if len(V) else None, len(V),
                                  float(th))
    n = len(pts)
    return rc, [dict(match_key=o["match_key"][:n], replace=o["replace"][:n], added=o["added"][:n], n_fused=int(V[v]["n_fused"]))
                for v, o in enumerate(out)]


def FuseScw(kfs, points, ids, visits, th=TH_SCW_FUSE):
    """int ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) for every visit (key frame index, Scw) of the list in
    one call.  returns per visit dict(match_key [n_points, n_cams] -- vnMatch as the best key per camera, -1 none --,
    replace [n_points] -- vpReplacePoint as the id the key frame's key held, -1 NULL --, added [n_points, n_cams] -- 1 where
    the reference calls AddObservation / AddMapPoint for match_key --, n_fused).
    One visit is the reference's Fuse exactly.  Several visits in one call are all searched with the tables as given at
    the call and each classified against its own key frame's mp_id at the call: what Replace() after key frame k changes
    in later key frames' map points, and the descriptor ComputeDistinctiveDescriptors may then give a loop point, are not
    seen.  A caller who wants the reference's sequence calls with one visit at a time."""
    rc, out = fuse_scw_call(kfs, points, ids, visits, th)
    _lib.check(rc, "vieo_fuse_scw")
    return out


def fuse_scw_tap(n_points, n_cams, visit):
    """the device stage of the last FuseScw: (best_idx, best_dist) int32[n_points, n_cams] before the threshold"""
    bi = np.zeros((max(n_points, 1), n_cams), np.int32)
    bd = np.zeros_like(bi)
    _lib.check(_lib.lib().vieo_fuse_scw_tap(visit, bi.ctypes.data, bd.ctypes.data), "vieo_fuse_scw_tap")
    return bi[:n_points], bd[:n_points]


def scw_gate_stats():
    """(items = visits x points x cameras, survivors of the gates) of the last SearchByProjectionScw / FuseScw"""
    a, b = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(_lib.lib().vieo_scw_gate_stats(ctypes.byref(a), ctypes.byref(b)), "vieo_scw_gate_stats")
    return a.value, b.value


def SearchAndFuse(kfs, Scws, points, ids, th=TH_SCW_FUSE):
    """The searches of LoopClosing::SearchAndFuse (LoopClosing.cc:682-707): Fuse(pKF, Scw, mvpLoopMapPoints, 4,
    vpReplacePoints) of every corrected key frame kfs[i] with its Scws[i], in one call.  returns per key frame what the
    caller must apply: dict(replace = [(id the key frame held, loop point index)] -- pRep->Replace(mvpLoopMapPoints[i]) --,
    add = [(loop point index, key)] -- the AddObservation / AddMapPoint pairs --, n_fused).  Replace and the map stay the
    caller's; see FuseScw for what several key frames in one call cannot see of each other."""
    out = FuseScw(kfs, points, ids, [(i, S) for i, S in enumerate(Scws)], th)
    res = []
    for o in out:
        rep = [(int(r), int(m)) for m, r in enumerate(o["replace"]) if r >= 0]
        add = [(int(m), int(o["match_key"][m, c])) for m, c in zip(*np.nonzero(o["added"]))]
        res.append(dict(replace=rep, add=add, n_fused=o["n_fused"]))
    return res


def sim3_world_pose(kf2, s12, R12, t12):
    """mg2oScw = gScm * gSmw (LoopClosing.cc:422-425) in double, gSmw = (R2w, t2w, 1): (s, R (3, 3), t (3,)) and the float
    3 x 4 mScw = s R | t"""
    R2, t2 = kf2.Rcw.astype(np.float64), kf2.tcw.astype(np.float64)
    s, R12, t12 = float(s12), np.asarray(R12, np.float64).reshape(3, 3), np.asarray(t12, np.float64)
    R, t = R12 @ R2, s * (R12 @ t2) + t12
    return s, R, t, np.concatenate([s * R, t[:, None]], axis=1).astype(np.float32)


def _copy_kf(kf, keys=None, desc=None, mp_id=None, cam_of_key=None, points=None, feat_vec=None):
    """a LoopKeyFrame with the pose, rig and pyramid of kf and other key arrays"""
    pick = lambda a, b: b if a is None else a
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = kf.Rcw, kf.tcw
    Tcr = []
    for c in range(kf.n_cams):
        M = np.eye(4)
        M[:3, :] = kf.Tcr[c].reshape(3, 4)
        Tcr.append(M)
    bow = BowKeys(pick(keys, kf.keys), pick(desc, kf.desc), pick(feat_vec, kf.bow.feat_vec), pick(mp_id, kf.mp_id))
    return LoopKeyFrame(bow, pick(points, kf.points), T, pick(cam_of_key, kf.cam_of_key), kf.cams, Tcr,
                        (float(kf.bounds[0][1]), float(kf.bounds[0][3])), kf.use_distort, kf.n_levels)


def make_loop_close_scene(seed, n_keys=200, n_points=120, n_cams=1, n_cands=2, free_share=0.3, plant=True):
    """A loop closure on top of make_loop_pair_scene(seed, ...): the current key frame (its map drifted by a similarity),
    n_cands candidates in the real world, the loop-point table drawn from the candidates -- every map point of every
    candidate once, candidate by candidate, in key order --, and the key frames SearchAndFuse corrects with their Scw: the
    current key frame through S12 of candidate 0 (sim3_world_pose) and the candidates through their own pose times a scale.
    free_share of the keys that hold a point lose it in every key frame (keys the searches may add to).
    plant: groups of extra loop points and extra keys of camera 0 of the current key frame at pixels of their own (octave 2,
    the level predicted for the point; every key within 9 px of it, inside the 14.4 px window of th = 10), named in
    `planted`:
      taken      three points at one place with one descriptor and two keys at distances 5 and 20: the first takes the
                 nearer key, the second the other one, the third finds both taken
      tie        a point with two keys at distance 7
      edge       a point with a key at distance 50 and one with a key at distance 51
      crowd      a point with 70 keys of one grid column within 5 px, each at a distance <= 30
      cone       two points whose normals stand 0.1 per mille inside and outside the 60 degree viewing cone
    and on a rig, in the corrected candidates, `two_ids` = [(index in fuse_kfs, key, larger key, its new id)]: map points
    held by a key in each camera whose larger key is given a map point of its own.
    returns dict(kf1 -- the current key frame, searched by SearchByProjectionScw --, kf2s, sim3, pairs, points, ids,
    Scw (3 x 4 float, of kf1), matched (int32[n_keys1]: the ids a third of the true pairs of candidate 0 give), fuse_kfs,
    fuse_Scws, planted)."""
    from .orb_extractor import KEYPOINT_DTYPE
    base = make_loop_pair_scene(seed, n_keys=n_keys, n_points=n_points, n_cams=n_cams, n_cands=n_cands)
    rng = np.random.default_rng(seed + 77)
    kf1, kf2s = base["kf1"], base["kf2s"]

    def flip(d, nbits):
        d = d.copy()
        for b in rng.choice(256, nbits, replace=False):
            d[b // 8] ^= np.uint8(1 << (b % 8))
        return d

    # the loop points: the candidates' map points
    points, ids, seen = [], [], set()
    for kf in kf2s:
        for i in np.flatnonzero(kf.mp_id >= 0):
            if int(kf.mp_id[i]) not in seen:
                seen.add(int(kf.mp_id[i]))
                points.append(kf.points[i].copy())
                ids.append(int(kf.mp_id[i]))
    s, R, t, Scw = sim3_world_pose(kf2s[0], *base["sim3"][0])
    matched = np.full(len(kf1.keys), -1, np.int32)
    for n, (i1, i2) in enumerate(sorted(base["pairs"][0].items())):
        if n % 3 == 0:
            matched[i1] = kf2s[0].mp_id[i2]

    def drop(kf):
        mp = kf.mp_id.copy()
        held = np.flatnonzero(mp >= 0)
        mp[rng.choice(held, int(free_share * len(held)), replace=False)] = -1
        return mp

    keys1, desc1, cam1, mp1, pts1 = kf1.keys.copy(), kf1.desc.copy(), kf1.cam_of_key.copy(), drop(kf1), kf1.points.copy()
    planted = {}
    if plant:
        # the corrected pose of the current key frame as the searches decompose it (in double: the margins below are wide)
        Rc, tc = R, t / s
        Oc = -Rc.T @ tc
        cam = kf1.cams[0]
        W, H = float(kf1.bounds[0][1]), float(kf1.bounds[0][3])
        col = W / 64.0
        new_keys, new_desc, next_id = [], [], [90000]

        def place(ix, v, angle_cos=1.0):
            """a loop point that projects to the centre of grid column ix at row v, 8 m away, predicted level 2"""
            u = ix * col
            if n_cams == 1:
                ray = np.array([(u - float(cam["cx"])) / float(cam["fx"]), (v - float(cam["cy"])) / float(cam["fy"]), 1.0])
            else:  # (a distorted camera: the pixel is only approximate, the keys are placed from the true projection)
                ray = np.array([(u - float(cam["cx"])) / float(cam["fx"]) * 0.5, (v - float(cam["cy"])) / float(cam["fy"]) * 0.5, 1.0])
            Xc = 8.0 * ray
            Xw = Rc.T @ (Xc - tc)
            if n_cams > 1:
                uv = _project_f64(kf1.cams, [np.vstack([kf1.Tcr[c].reshape(3, 4), [0, 0, 0, 1]]) for c in range(n_cams)], Xc, 0)
                u, v = uv
            d = np.linalg.norm(Xw - Oc)
            direction = (Xw - Oc) / d
            perp = np.cross(direction, [0.3, -0.5, 0.8])
            perp /= np.linalg.norm(perp)
            P = np.zeros(1, FUSE_POINT_DTYPE)[0]
            P["Xw"], P["normal"] = Xw, angle_cos * direction + np.sqrt(1 - angle_cos ** 2) * perp
            P["max_distance"] = d * 1.2 ** 1.5
            P["min_distance"] = P["max_distance"] / np.float32(1.2 ** 7)
            P["desc"] = rng.integers(0, 256, 32, dtype=np.uint8)
            return P, (u, v)

        def add_point(P):
            points.append(P.copy())
            ids.append(next_id[0])
            next_id[0] += 1
            return len(points) - 1

        def add_key(uv, desc, dx=0.0, dy=0.0):
            k = np.zeros(1, KEYPOINT_DTYPE)[0]
            k["x"], k["y"], k["octave"], k["size"], k["angle"] = uv[0] + dx, uv[1] + dy, 2, 31.0, 0.0
            new_keys.append(k)
            new_desc.append(desc)
            return len(keys1) + len(new_keys) - 1

        P, uv = place(8, 60.0)
        ka, kb = add_key(uv, flip(P["desc"], 5), 1.0), add_key(uv, flip(P["desc"], 20), -1.0)
        planted["taken"] = dict(points=[add_point(P), add_point(P), add_point(P)], keys=[ka, kb])
        P, uv = place(14, 60.0)
        planted["tie"] = dict(point=add_point(P), keys=[add_key(uv, flip(P["desc"], 7), 1.5), add_key(uv, flip(P["desc"], 7), -1.5)])
        P, uv = place(20, 60.0)
        Q, uvq = place(26, 60.0)
        planted["edge"] = dict(points=[add_point(P), add_point(Q)], keys=[add_key(uv, flip(P["desc"], 50)), add_key(uvq, flip(Q["desc"], 51))])
        P, uv = place(32, 60.0)
        mid = (round(uv[0] / col) * col, uv[1])  # the centre of the grid column the point falls into
        crowd = [add_key(mid, flip(P["desc"], int(rng.integers(0, 31))), rng.uniform(-2, 2), rng.uniform(-5, 5)) for _ in range(70)]
        planted["crowd"] = dict(point=add_point(P), keys=crowd)
        P, uv = place(38, 60.0, 0.5 * (1 + 1e-4))
        Q, uvq = place(44, 60.0, 0.5 * (1 - 1e-4))
        planted["cone"] = dict(points=[add_point(P), add_point(Q)], keys=[add_key(uv, flip(P["desc"], 3)), add_key(uvq, flip(Q["desc"], 3))])
        m = len(new_keys)
        keys1 = np.concatenate([keys1, np.array(new_keys, KEYPOINT_DTYPE)])
        desc1 = np.concatenate([desc1, np.stack(new_desc)])
        cam1 = np.concatenate([cam1, np.zeros(m, np.int32)])
        mp1 = np.concatenate([mp1, np.full(m, -1, np.int32)])
        pts1 = np.concatenate([pts1, np.zeros(m, FUSE_POINT_DTYPE)])
        matched = np.concatenate([matched, np.full(m, -1, np.int32)])
    # (the key frame SearchByProjectionScw reads: every key it holds a point at keeps it -- vpMatched is what counts there)
    kf1_search = _copy_kf(kf1, keys1, desc1, np.concatenate([kf1.mp_id, np.full(len(keys1) - len(kf1.keys), -1, np.int32)]),
                          cam1, pts1)
    fuse_kfs = [_copy_kf(kf1, keys1, desc1, mp1, cam1, pts1)]
    fuse_Scws = [Scw]
    for c, kf in enumerate(kf2s):
        mp = drop(kf)
        if n_cams > 1:  # a map point held by a key in each camera: the larger key gets a map point of its own
            held = {}
            for k, m_ in enumerate(mp):
                if m_ >= 0:
                    held.setdefault(int(m_), []).append(k)
            for ka, kb in [ks for ks in held.values() if len(ks) == 2][:3]:
                mp[kb] = 95000 + 10 * c + len(planted.setdefault("two_ids", []))
                planted["two_ids"].append((1 + c, ka, kb, int(mp[kb])))
        fuse_kfs.append(_copy_kf(kf, mp_id=mp))
        sc = 1.0 + 0.01 * (c + 1)
        fuse_Scws.append((sc * np.concatenate([kf.Rcw.astype(np.float64), kf.tcw.astype(np.float64)[:, None]], axis=1)).astype(np.float32))
    return dict(kf1=kf1_search, kf2s=kf2s, sim3=base["sim3"], pairs=base["pairs"], points=np.array(points, FUSE_POINT_DTYPE),
                ids=np.array(ids, np.int32), Scw=Scw, matched=matched, fuse_kfs=fuse_kfs, fuse_Scws=fuse_Scws, planted=planted)


# ---------------------------------------------------------------------------------------------------------------------
# LoopClosing::ComputeSim3 as one call
COMPUTE_SIM3_VISIT_DTYPE = np.dtype([(name, "<i4") for name in ("cand", "call", "row", "no_more", "found", "n_inliers", "n_found",
                                                                "n_opt_inliers")])
COMPUTE_SIM3_RESULT_DTYPE = np.dtype([("found", "<i4"), ("cand", "<i4"), ("n_inliers", "<i4"), ("n_visits", "<i4"), ("s", "<f8"),
                                      ("R", "<f8", 9), ("t", "<f8", 3), ("Scw", "<f4", 12)], align=True)
assert COMPUTE_SIM3_VISIT_DTYPE.itemsize == 32 and COMPUTE_SIM3_RESULT_DTYPE.itemsize == 168
THRESH_MATCHES, THRESH_INLIERS = 20, 20  # the reference's defaults of thresh_matches_[0] / thresh_inliers_[0]


def compute_sim3_call(kf1, cands, thresh_matches=THRESH_MATCHES, min_inliers=THRESH_INLIERS, fix_scale=False, samples=None,
                      n_rows=300, seed=0, trace_capacity=4096):
    """vieo_compute_sim3, raw.  samples: a list of n_cands arrays (S, 3) (a candidate that gets no solver may have any
    valid-looking rows), or None to let the library draw n_rows rows from `seed`.  returns (rc, dict(found, cand, n_inliers,
    s, R (3, 3), t, Scw (3, 4) float32, match12 int32[n_keys1], n_visits, trace = [(cand, call, row, no_more, found,
    n_inliers, n_found, n_opt_inliers)]))"""
    recs = np.concatenate([k.rec for k in cands]) if cands else np.zeros(0, LOOP_KEYFRAME_DTYPE)
    if samples is not None:
        samples = np.ascontiguousarray(np.stack([np.asarray(s, np.int32).reshape(-1, 3) for s in samples]))
        n_rows = samples.shape[1]
    res = np.zeros(1, COMPUTE_SIM3_RESULT_DTYPE)
    match12 = np.full(max(len(kf1.keys), 1), -7, np.int32)
    trace = np.zeros(max(trace_capacity, 1), COMPUTE_SIM3_VISIT_DTYPE)
    rc = _lib.lib().vieo_compute_sim3(kf1.rec.ctypes.data, recs.ctypes.data if len(recs) else None, len(cands), int(thresh_matches),
                                      int(min_inliers), int(bool(fix_scale)), samples.ctypes.data if samples is not None else None,
                                      int(n_rows), int(seed), res.ctypes.data, match12.ctypes.data, trace.ctypes.data,
                                      int(trace_capacity))
    r = res[0]
    n = min(int(r["n_visits"]), trace_capacity)
    return rc, dict(found=bool(r["found"]), cand=int(r["cand"]), n_inliers=int(r["n_inliers"]), s=float(r["s"]),
                    R=r["R"].reshape(3, 3).copy(), t=r["t"].copy(), Scw=r["Scw"].reshape(3, 4).copy(),
                    match12=match12[:len(kf1.keys)], n_visits=int(r["n_visits"]), trace=[tuple(int(x) for x in row) for row in trace[:n]])


def ComputeSim3(kf1, cands, loop_points_of, thresh_matches=THRESH_MATCHES, min_inliers=THRESH_INLIERS, fix_scale=False,
                samples=None, n_rows=300, seed=0):
    """bool LoopClosing::ComputeSim3() (LoopClosing.cc:308-489): vieo_compute_sim3 -- SearchByBoW of every candidate, the
    Sim3Solver of the kept ones, the round-robin of iterate(5) / SearchBySim3 / OptimizeSim3 --, then loop_points_of(index of
    the matched candidate) -> (points FUSE_POINT_DTYPE, ids), the caller's gather of :446-463, then SearchByProjection(
    mpCurrentKF, mScw, mvpLoopMapPoints, mvpCurrentMatchedPoints, 10) and nTotalMatches >= 40.
    returns (the reference's bool, dict(cand, Scw (3, 4) float32, s, R, t, matched int32[n_keys1] -- mvpCurrentMatchedPoints as
    ids, -1 NULL --, n_total_matches, trace)); cand is -1 and matched all -1 when no candidate matched."""
    rc, o = compute_sim3_call(kf1, cands, thresh_matches, min_inliers, fix_scale, samples, n_rows, seed)
    _lib.check(rc, "vieo_compute_sim3")
    out = dict(cand=o["cand"], Scw=o["Scw"], s=o["s"], R=o["R"], t=o["t"], trace=o["trace"], n_total_matches=0,
               matched=np.full(len(kf1.keys), -1, np.int32))
    if not o["found"]:
        return False, out
    kf2, m = cands[o["cand"]], o["match12"]
    matched = np.where(m >= 0, kf2.mp_id[np.maximum(m, 0)], -1).astype(np.int32)
    points, ids = loop_points_of(o["cand"])
    (matched, _), = SearchByProjectionScw([kf1], points, ids, [(0, o["Scw"], matched)], TH_SCW_SEARCH)
    out["matched"], out["n_total_matches"] = matched, int((matched >= 0).sum())
    return out["n_total_matches"] >= LOOP_MATCHES, out


def make_compute_sim3_scene(seed, n_cands=2, fail=False, n_keys=200, n_points=120, n_nodes=30):
    """make_loop_pair_scene(seed, ...) made fit for the whole of ComputeSim3: every key in a vocabulary node (a physical
    point's keys share one, so SearchByBoW can pair them; keys without a point lie in random nodes), key angles that agree
    between the key frames up to one rotation per candidate (the orientation histogram keeps the pairs), and in every
    candidate six pairs of keys of one node with their descriptors exchanged: SearchByBoW pairs each with the other's
    physical point, an outlier of the RANSAC.
    fail: candidate 0 lies in nodes of its own (no match at all) and the map points of candidate 1 are shuffled among its
    keys (enough matches, no consensus): every candidate is discarded.
    Physical points j and j + 1000 share node and angle (the ids of make_loop_pair_scene repeat there): more than 1000
    points only crowd the nodes.
    returns dict(kf1, kf2s, sim3, pairs, loop_points_of) -- loop_points_of(c): the map points of candidate c, once each."""
    base = make_loop_pair_scene(seed, n_keys=n_keys, n_points=n_points, n_cands=n_cands)
    rng = np.random.default_rng(seed + 131)
    nodes = np.sort(rng.choice(100000, 2 * n_nodes, replace=False))
    node_of_phys = rng.integers(0, n_nodes, 1000)
    angle_of_phys = rng.uniform(0, 360, 1000)

    def remake(kf, rot, own_nodes=False, swaps=0, shuffle_points=False):
        phys = np.where(kf.mp_id >= 0, kf.mp_id % 1000, -1)
        node = np.where(phys >= 0, node_of_phys[np.maximum(phys, 0)], rng.integers(0, n_nodes, len(phys)))
        if own_nodes:
            node = node + n_nodes
        keys, desc, points = kf.keys.copy(), kf.desc.copy(), kf.points.copy()
        ang = np.where(phys >= 0, (angle_of_phys[np.maximum(phys, 0)] - rot + rng.normal(0, 1.0, len(phys))) % 360.0, keys["angle"])
        keys["angle"] = np.where(ang >= 359.99, 0.0, ang)
        done = 0
        for n in range(n_nodes):  # exchange the descriptors of two keys of a node that hold different points
            held = [int(i) for i in np.flatnonzero((node == n) & (phys >= 0))]
            if done < swaps and len(held) >= 2 and phys[held[0]] != phys[held[1]]:
                desc[[held[0], held[1]]] = desc[[held[1], held[0]]]
                done += 1
        if shuffle_points:
            held = np.flatnonzero(phys >= 0)
            points[held] = points[rng.permutation(held)]
        fv = [(int(nodes[n]), [int(i) for i in np.flatnonzero(node == n)]) for n in np.unique(node)]
        return _copy_kf(kf, keys=keys, desc=desc, points=points, feat_vec=fv)

    kf1 = remake(base["kf1"], 0.0)
    kf2s = [remake(kf, rng.uniform(0, 360), own_nodes=fail and c == 0, swaps=0 if fail else 6, shuffle_points=fail and c == 1)
            for c, kf in enumerate(base["kf2s"])]

    def loop_points_of(c):
        kf, seen, idx = kf2s[c], set(), []
        for i in np.flatnonzero(kf.mp_id >= 0):
            if int(kf.mp_id[i]) not in seen:
                seen.add(int(kf.mp_id[i]))
                idx.append(int(i))
        return kf.points[idx].copy(), kf.mp_id[idx].copy()
    return dict(kf1=kf1, kf2s=kf2s, sim3=base["sim3"], pairs=base["pairs"], loop_points_of=loop_points_of)
