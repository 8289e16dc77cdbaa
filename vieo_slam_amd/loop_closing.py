"""Loop verification on the device, first half (reference LoopClosing::ComputeSim3, src/LoopClosing.cc:308-489): what it
does for every candidate before any decision depends on another one.  SearchByBoWKF -- ORBmatcher::SearchByBoW(KeyFrame*,
KeyFrame*) of the current key frame against all candidates in one call --, Sim3Solver -- the reference's Sim3Solver for
a batch of candidates (every RANSAC hypothesis of every candidate in one launch, iterate / find / GetEstimated* as
look-ups) -- with draw_samples and sim3_correspondences (the constructor on flat key-frame arrays), and make_sim3_scene /
make_bow_kf_scene, the generators of the tests and of tools/time_loop_sim3.py.  SearchBySim3, OptimizeSim3 and the
round-robin loop of ComputeSim3 are not here."""
import ctypes

import numpy as np

from . import _lib
from .ba_types import CAMERA_DTYPE
from .relocalization import CAMERA_K, HEIGHT, WIDTH, BowKeys, _unpack_masks, rodrigues
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
