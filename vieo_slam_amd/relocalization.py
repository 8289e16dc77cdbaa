"""Relocalisation of a lost frame on the device (reference Tracking::Relocalization, src/Tracking.cc:2529-2686):
SearchByBoW -- ORBmatcher::SearchByBoW(KeyFrame*, Frame&) of all candidate key frames in one call --, PnPSolver --
PnPsolver for a batch of candidates (every RANSAC hypothesis of every candidate in one launch, Refine in a second,
PnPsolver::iterate as look-ups) -- with draw_samples, and make_pnp_scene / make_bow_scene, the generators of the tests
and of tools/time_relocalization.py.  A frame of a 1- to 4-camera rig (Frame::usedistort_) has its own forms: SearchByBoWRig,
PnPSolver(..., rig=, cam_of=) with usun(), RelocRig / RelocalizationRig, and the generators make_bow_rig_scene,
make_pnp_rig_scene, make_reloc_rig_scene on the rigs of the rig pipeline tests (rig_of: "radtan2", "kb8x4")."""
import ctypes
import math

import numpy as np

from . import _lib

MAX_ROWS = 512

PNP_CANDIDATE_DTYPE = np.dtype([("n", np.int32), ("n_frame_keys", np.int32), ("Xw", np.uint64), ("uv", np.uint64),
                                ("sigma2", np.uint64), ("key_index", np.uint64), ("fx", np.float32), ("fy", np.float32),
                                ("cx", np.float32), ("cy", np.float32)], align=True)
PNP_PARAMS_DTYPE = np.dtype([("probability", np.float64), ("min_inliers", np.int32), ("max_iterations", np.int32),
                             ("min_set", np.int32), ("epsilon", np.float32), ("th2", np.float32), ("reserved", np.int32)],
                            align=True)
PNP_INFO_DTYPE = np.dtype([("n", np.int32), ("n_frame_keys", np.int32), ("min_inliers", np.int32), ("max_its", np.int32),
                           ("n_rows", np.int32), ("n_records", np.int32), ("mask_words", np.int32), ("iterations", np.int32),
                           ("best_inliers", np.int32), ("best_row", np.int32)], align=True)



def _pnp_rig_dtype():
    from .ba_types import CAMERA_DTYPE
    return np.dtype([("n_cams", np.int32), ("reserved", np.int32), ("cams", CAMERA_DTYPE, 4), ("Tcr", np.float64, (4, 12)),
                     ("Trc", np.float64, (4, 12))], align=True)


PNP_RIG_DTYPE = _pnp_rig_dtype()  # vieo_pnp_rig
RELOC_RIG_DTYPE = np.dtype([("pnp", PNP_RIG_DTYPE), ("cam_first", np.uint64), ("sbp", np.uint64), ("pose_cams", np.uint64)],
                           align=True)  # vieo_reloc_rig


def make_pnp_rig(cams, Tcr):
    """PNP_RIG_DTYPE[1] from a CAMERA_DTYPE array and the list of 4 x 4 Tcr (reference camera -> camera c).  Tcr / Trc
    go through Sophus::SE3<float> like the camera members (synth_fisheye.rig_extrinsics)."""
    from .synth_fisheye import rig_extrinsics
    rig = np.zeros(1, PNP_RIG_DTYPE)
    nc = len(cams)
    Trc_a, Tcr_a = rig_extrinsics(Tcr)
    rig["n_cams"] = nc
    rig["cams"][0, :nc] = cams
    rig["Tcr"][0, :nc], rig["Trc"][0, :nc] = Tcr_a, Trc_a
    return rig


# Tracking.cc:2572: pSolver->SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991)
RELOC_PNP_PARAMS = dict(probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, th2=5.991)


def draw_samples(rng, n, n_rows, set_size=4):
    """n_rows minimal sets of set_size indices < n (4: PnPsolver; 3: Sim3Solver), each drawn without replacement the way
    PnPsolver::iterate does (PnPsolver.cc:174-186): a uniform position in the list of available indices, whose entry is
    then overwritten by the list's last one.  rng: numpy Generator (the reference draws through rand())."""
    out = np.empty((n_rows, set_size), np.int32)
    for r in range(n_rows):
        avail = list(range(n))
        for i in range(set_size):
            k = int(rng.integers(0, len(avail)))
            out[r, i] = avail[k]
            avail[k] = avail[-1]
            avail.pop()
    return out


def _params_record(params):
    p = dict(RELOC_PNP_PARAMS)
    p.update(params or {})
    rec = np.zeros(1, PNP_PARAMS_DTYPE)
    for k, v in p.items():
        rec[k] = v
    return rec


def _unpack_masks(words, n):
    """(m, mask_words) uint64 -> (m, n) bool, bit i of the mask = correspondence i"""
    words = np.ascontiguousarray(words, np.uint64)
    bits = np.unpackbits(words.view(np.uint8).reshape(len(words), -1), axis=1, bitorder="little")
    return bits[:, :n].astype(bool)


def _pack_masks(masks):
    masks = np.atleast_2d(np.asarray(masks, bool))
    n = masks.shape[1]
    words = (n + 63) // 64
    padded = np.zeros((len(masks), words * 64), np.uint8)
    padded[:, :n] = masks
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint64).reshape(len(masks), words)


class _Candidate:
    def __init__(self, Xw, uv, sigma2, key_index, n_frame_keys, K):
        self.Xw = np.ascontiguousarray(Xw, np.float32).reshape(-1, 3)
        self.uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        self.sigma2 = np.ascontiguousarray(sigma2, np.float32).reshape(-1)
        self.key_index = np.ascontiguousarray(key_index, np.int32).reshape(-1)
        self.n_frame_keys = int(n_frame_keys)
        self.K = tuple(float(k) for k in K)
        n = len(self.Xw)
        if not (len(self.uv) == len(self.sigma2) == len(self.key_index) == n):
            raise ValueError("PnPSolver: Xw, uv, sigma2 and key_index differ in length")

    def record(self):
        rec = np.zeros(1, PNP_CANDIDATE_DTYPE)
        rec["n"], rec["n_frame_keys"] = len(self.Xw), self.n_frame_keys
        rec["Xw"], rec["uv"] = self.Xw.ctypes.data, self.uv.ctypes.data
        rec["sigma2"], rec["key_index"] = self.sigma2.ctypes.data, self.key_index.ctypes.data
        rec["fx"], rec["fy"], rec["cx"], rec["cy"] = self.K
        return rec


class PnPResult:
    def __init__(self, found, Tcw, inliers, n_inliers, no_more, row):
        self.found, self.Tcw, self.inliers, self.n_inliers, self.no_more, self.row = found, Tcw, inliers, n_inliers, no_more, row


class PnPSolver:
    """PnPsolver of K relocalisation candidates at once.

    candidates: a list of dicts with Xw (n, 3), uv (n, 2), sigma2 (n,), key_index (n,), n_frame_keys and K = (fx, fy, cx,
    cy) -- what PnPsolver's constructor collects from the frame and vpMapPointMatches.  samples: (K, S, 4) indices from
    draw_samples (a list of K arrays (S, 4) will do), or None to let the library draw from `seed`.  All hypotheses are
    evaluated when the object is made; iterate(c, n) is PnPsolver::iterate of candidate c.

    A frame of a camera rig (Frame::usedistort_): rig = a PNP_RIG_DTYPE record (make_pnp_rig) and cam_of = per candidate
    the camera of every correspondence (mapidx2cami_; default: the candidates' "cam_of"); uv are then the mvKeys pixels
    and K is camera 0's toK().  usun(c) gives what fill_M reads."""

    def __init__(self, candidates, samples=None, n_rows=None, seed=0, params=None, rig=None, cam_of=None):
        self._h = None
        self._cands = [_Candidate(c["Xw"], c["uv"], c["sigma2"], c["key_index"], c["n_frame_keys"], c["K"])
                       for c in candidates]
        K = len(self._cands)
        self._rig = None if rig is None else np.ascontiguousarray(rig, PNP_RIG_DTYPE).reshape(1)
        if rig is not None:
            cam_of = [c["cam_of"] for c in candidates] if cam_of is None else cam_of
            self._cam_of = [np.ascontiguousarray(a, np.uint8).reshape(-1) for a in cam_of]
            if [len(a) for a in self._cam_of] != [len(c.Xw) for c in self._cands]:
                raise ValueError("PnPSolver: cam_of differs in length from the correspondences")
            self._cam_ptr = np.array([a.ctypes.data for a in self._cam_of], np.uint64)
        if samples is not None:
            samples = np.ascontiguousarray(np.stack([np.asarray(s, np.int32).reshape(-1, 4) for s in samples]))
            n_rows = samples.shape[1]
        elif n_rows is None:
            raise ValueError("PnPSolver: pass samples or n_rows")
        self.n_rows = int(n_rows)
        recs = np.concatenate([c.record() for c in self._cands]) if K else np.zeros(0, PNP_CANDIDATE_DTYPE)
        par = _params_record(params)
        h = ctypes.c_void_p()
        smp = samples.ctypes.data if samples is not None else None
        if rig is None:
            rc = _lib.lib().vieo_pnp_create(ctypes.byref(h), recs.ctypes.data, K, par.ctypes.data, smp, self.n_rows, int(seed))
            _lib.check(rc, "vieo_pnp_create")
        else:
            rc = _lib.lib().vieo_pnp_create_rig(ctypes.byref(h), recs.ctypes.data, K, self._cam_ptr.ctypes.data,
                                                self._rig.ctypes.data, par.ctypes.data, smp, self.n_rows, int(seed))
            _lib.check(rc, "vieo_pnp_create_rig")
        self._h = h

    def close(self):
        if self._h:
            _lib.lib().vieo_pnp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self, c):
        rec = np.zeros(1, PNP_INFO_DTYPE)
        _lib.check(_lib.lib().vieo_pnp_get_info(self._h, c, rec.ctypes.data), "vieo_pnp_get_info")
        return {k: int(rec[k][0]) for k in PNP_INFO_DTYPE.names}

    def iterate(self, c, n_iterations):
        cand = self._cands[c]
        found, n_inl, no_more, row = (ctypes.c_int32() for _ in range(4))
        Tcw = np.zeros((4, 4), np.float32)
        inl = np.zeros(max(cand.n_frame_keys, 1), np.uint8)
        rc = _lib.lib().vieo_pnp_iterate(self._h, c, int(n_iterations), ctypes.byref(found), Tcw.ctypes.data, inl.ctypes.data,
                                         ctypes.byref(n_inl), ctypes.byref(no_more), ctypes.byref(row))
        if rc == _lib.VIEO_E_CAPACITY:  # the sample table is used up: reported like bNoMore, as vieo_relocalize takes it
            return PnPResult(False, None, None, 0, 2, -1)
        _lib.check(rc, "vieo_pnp_iterate")
        ok = bool(found.value)
        return PnPResult(ok, Tcw if ok else None, inl[:cand.n_frame_keys].astype(bool) if ok else None, n_inl.value,
                         bool(no_more.value), row.value)

    def rows(self, c):
        """test tap, pass A: samples (S, 4), Rt (S, 12) = R row-major then t, count (S,), mask (S, n) bool"""
        i, S = self.info(c), self.n_rows
        smp, Rt, cnt = np.zeros((S, 4), np.int32), np.zeros((S, 12)), np.zeros(S, np.int32)
        words = np.zeros((S, max(i["mask_words"], 1)), np.uint64)
        _lib.check(_lib.lib().vieo_pnp_tap_rows(self._h, c, smp.ctypes.data, Rt.ctypes.data, cnt.ctypes.data, words.ctypes.data),
                   "vieo_pnp_tap_rows")
        return smp, Rt, cnt, _unpack_masks(words, i["n"])

    def records(self, c):
        """test tap, pass B: rec_row (r,), Rt (r, 12), count (r,), mask (r, n) bool"""
        i = self.info(c)
        r = i["n_records"]
        row, Rt, cnt = np.zeros(max(r, 1), np.int32), np.zeros((max(r, 1), 12)), np.zeros(max(r, 1), np.int32)
        words = np.zeros((max(r, 1), max(i["mask_words"], 1)), np.uint64)
        _lib.check(_lib.lib().vieo_pnp_tap_records(self._h, c, row.ctypes.data, Rt.ctypes.data, cnt.ctypes.data,
                                                   words.ctypes.data), "vieo_pnp_tap_records")
        return row[:r], Rt[:r], cnt[:r], _unpack_masks(words, i["n"])[:r]

    def usun(self, c):
        """test tap, rig solvers: usun (n, 2) float64 of candidate c (add_correspondence: un-project, Trc, K0, divide)"""
        out = np.zeros((max(len(self._cands[c].Xw), 1), 2))
        _lib.check(_lib.lib().vieo_pnp_tap_usun(self._h, c, out.ctypes.data), "vieo_pnp_tap_usun")
        return out[:len(self._cands[c].Xw)]

    @staticmethod
    def refine_masks(candidate, masks, params=None, rig=None, cam_of=None):
        """test tap: pass B alone (Refine: EPnP over a given inlier set, then CheckInliers) on masks (m, n) bool; with
        rig (and cam_of, default the candidate's "cam_of") the rig instance"""
        c = _Candidate(candidate["Xw"], candidate["uv"], candidate["sigma2"], candidate["key_index"],
                       candidate["n_frame_keys"], candidate["K"])
        words = _pack_masks(masks)
        m = len(words)
        Rt, cnt, out = np.zeros((m, 12)), np.zeros(m, np.int32), np.zeros_like(words)
        rec, par = c.record(), _params_record(params)
        if rig is None:
            rc = _lib.lib().vieo_pnp_tap_refine(rec.ctypes.data, par.ctypes.data, words.ctypes.data, m, Rt.ctypes.data,
                                                cnt.ctypes.data, out.ctypes.data)
            _lib.check(rc, "vieo_pnp_tap_refine")
        else:
            cams = np.ascontiguousarray(candidate["cam_of"] if cam_of is None else cam_of, np.uint8).reshape(-1)
            assert len(cams) == len(c.Xw)
            rig = np.ascontiguousarray(rig, PNP_RIG_DTYPE).reshape(1)
            rc = _lib.lib().vieo_pnp_tap_refine_rig(rec.ctypes.data, cams.ctypes.data, rig.ctypes.data, par.ctypes.data,
                                                    words.ctypes.data, m, Rt.ctypes.data, cnt.ctypes.data, out.ctypes.data)
            _lib.check(rc, "vieo_pnp_tap_refine_rig")
        return Rt, cnt, _unpack_masks(out, len(c.Xw))


# ---------------------------------------------------------------------------------------------------------------------
# scenes
CAMERA_K = tuple(float(np.float32(v)) for v in (435.2, 435.2, 367.2, 252.2))  # 752 x 480
WIDTH, HEIGHT = 752, 480


def rodrigues(w):
    th = float(np.linalg.norm(w))
    if th == 0:
        return np.eye(3)
    k = np.asarray(w, np.float64) / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * (Kx @ Kx)


def make_pnp_scene(seed, n=60, outlier_share=0.15, pixel_noise=0.5, rng=None):
    """One candidate's correspondences: n map points at 1.5-12 m in front of a 752 x 480 pinhole camera whose true pose
    has a rotation vector ~ N(0, 0.15 rad) per axis and a translation ~ N(0, 0.3 m); keys on octaves 0..3 with
    sigma2 = 1.2^(2 octave) and pixel noise pixel_noise * 1.2^octave; outlier_share of the pixels replaced by uniform
    ones.  Xw and uv are rounded to float32 like mvP3Dw / mvP2D."""
    rng = np.random.default_rng(seed) if rng is None else rng
    fx, fy, cx, cy = CAMERA_K
    R, t = rodrigues(rng.standard_normal(3) * 0.15), rng.standard_normal(3) * 0.3
    u, v, z = rng.uniform(40, WIDTH - 40, n), rng.uniform(40, HEIGHT - 40, n), rng.uniform(1.5, 12.0, n)
    Pc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], axis=1)
    Xw = ((Pc - t) @ R).astype(np.float32)  # R^T (Pc - t)
    octave = rng.integers(0, 4, n)
    scale = 1.2 ** octave
    uv = np.stack([u, v], axis=1) + rng.standard_normal((n, 2)) * (pixel_noise * scale)[:, None]
    n_out = int(round(n * outlier_share))
    bad = rng.choice(n, n_out, replace=False)
    uv[bad] = np.stack([rng.uniform(0, WIDTH, n_out), rng.uniform(0, HEIGHT, n_out)], axis=1)
    truth = np.ones(n, bool)
    truth[bad] = False
    return dict(R=R, t=t, Xw=Xw, uv=uv.astype(np.float32), sigma2=(scale * scale).astype(np.float32),
                octave=octave.astype(np.int32), key_index=np.arange(n, dtype=np.int32), n_frame_keys=n, K=CAMERA_K,
                truth=truth)


RIG_KINDS = {"radtan2": ("radtan", 0.5), "kb8x4": ("kb8", 1.0)}  # synth_ba.camera_rig name, widest view angle drawn (rad)


def rig_of(rig_kind):
    """The rigs of the rig pipeline tests by the names of the benchmark's workloads: "radtan2" = the two EuRoC Radtan
    cameras, "kb8x4" = the four TUM-VI-like KB8 cameras (synth_ba.camera_rig).  returns dict(cams CAMERA_DTYPE[n],
    size (W, H), Tcr [4 x 4], Tcr_a / Trc_a (n, 3, 4) as the camera members hold them, pnp PNP_RIG_DTYPE[1], K =
    camera 0's toK(), theta_max)."""
    from . import synth_ba
    from .synth_fisheye import rig_extrinsics
    name, theta_max = RIG_KINDS[rig_kind]
    cams, size, Tcr = synth_ba.camera_rig(name, with_tcr=True)
    Trc_a, Tcr_a = rig_extrinsics(Tcr)
    K = tuple(float(cams[0][k]) for k in ("fx", "fy", "cx", "cy"))
    return dict(kind=rig_kind, cams=cams, size=size, Tcr=Tcr, Tcr_a=Tcr_a.reshape(-1, 3, 4), Trc_a=Trc_a.reshape(-1, 3, 4),
                pnp=make_pnp_rig(cams, Tcr), K=K, theta_max=theta_max)


def _rig_view(rig, c, Pr, margin=8.0):
    """pixel of the reference-camera point Pr in camera c of the rig, or None when it is behind the camera, outside the
    view angle drawn or outside the image"""
    from . import synth_ba
    W, H = rig["size"]
    Pc = rig["Tcr_a"][c][:, :3] @ Pr + rig["Tcr_a"][c][:, 3]
    if Pc[2] < 0.2 or np.arctan2(np.hypot(Pc[0], Pc[1]), Pc[2]) > rig["theta_max"]:
        return None
    u, v = synth_ba.project_camera(rig["cams"][c], Pc)
    return (u, v) if margin <= u < W - margin and margin <= v < H - margin else None


def _draw_rig_point(rng, rig, c, plane_z, margin):
    """A point in the view of camera c of the rig, 1.5-12 m from it, or -- plane_z given -- on the plane z = plane_z
    of that camera: (the point in the reference camera, its pixel in camera c)."""
    while True:
        th, ph, d = rng.uniform(0, rig["theta_max"]), rng.uniform(0, 2 * np.pi), rng.uniform(1.5, 12.0)
        if plane_z is not None:
            d = plane_z / np.cos(th)
        Pc = d * np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
        P = rig["Trc_a"][c][:, :3] @ Pc + rig["Trc_a"][c][:, 3]
        px = _rig_view(rig, c, P, margin)
        if px is not None:
            return P, px


def make_pnp_rig_scene(seed, rig_kind, n=60, outlier_share=0.15, pixel_noise=0.5, rng=None, held_twice=0,
                       plane_z=None):
    """make_pnp_scene for a frame of a camera rig: correspondence i belongs to camera i % n_cams, its map point lies
    1.5-12 m away inside that camera's view, uv is the camera model's projection (the mvKeys pixel) plus noise; the true
    pose R, t is that of the reference camera.  held_twice: the map points of correspondences 0, 2, ... 2 (held_twice - 1)
    are also held by the next correspondence, seen from another camera (a map point matched in two images).
    plane_z: every point on the plane z = plane_z of its own camera instead of 1.5-12 m away.  plane_z = 1 is the one
    place where the reference's usun -- the un-projected point on that plane moved by
    GetTrc() -- is the point's central projection in the reference camera; anywhere else a camera at a baseline b from
    the reference camera leaves usun a parallax of about fx b |1 - 1/z| pixels.
    returns make_pnp_scene's dict plus cam_of (n,) uint8, rig (rig_of), Pr (n, 3) the points in the reference camera."""
    rng = np.random.default_rng(seed) if rng is None else rng
    rig = rig_of(rig_kind)
    nc = len(rig["cams"])
    W, H = rig["size"]
    R, t = rodrigues(rng.standard_normal(3) * 0.15), rng.standard_normal(3) * 0.3
    cam_of = (np.arange(n) % nc).astype(np.uint8)
    Pr, uv = np.zeros((n, 3)), np.zeros((n, 2))
    for i in range(n):
        Pr[i], uv[i] = _draw_rig_point(rng, rig, int(cam_of[i]), plane_z, 8.0)
    for j in range(held_twice):
        a, b = 2 * j, 2 * j + 1
        for c in list(range(int(cam_of[a]) + 1, nc)) + list(range(int(cam_of[a]))):
            px = _rig_view(rig, c, Pr[a])
            if px is not None:
                Pr[b], uv[b], cam_of[b] = Pr[a], px, c
                break
        else:
            raise ValueError("make_pnp_rig_scene: point %d is seen by one camera only" % a)
    Xw = ((Pr - t) @ R).astype(np.float32)  # R^T (Pr - t)
    octave = rng.integers(0, 4, n)
    scale = 1.2 ** octave
    uv = uv + rng.standard_normal((n, 2)) * (pixel_noise * scale)[:, None]
    n_out = int(round(n * outlier_share))
    bad = rng.choice(n, n_out, replace=False)
    uv[bad] = np.stack([rng.uniform(0, W, n_out), rng.uniform(0, H, n_out)], axis=1)
    truth = np.ones(n, bool)
    truth[bad] = False
    return dict(R=R, t=t, Xw=Xw, uv=uv.astype(np.float32), sigma2=(scale * scale).astype(np.float32),
                octave=octave.astype(np.int32), key_index=np.arange(n, dtype=np.int32), n_frame_keys=n, K=rig["K"],
                truth=truth, cam_of=cam_of, rig=rig, Pr=Pr)


# ---------------------------------------------------------------------------------------------------------------------
# SearchByBoW
BOW_KEYS_DTYPE = np.dtype([("n_keys", np.int32), ("n_nodes", np.int32), ("keys", np.uint64), ("descriptors", np.uint64),
                           ("mp_id", np.uint64), ("node_id", np.uint64), ("node_first", np.uint64),
                           ("node_feat", np.uint64)], align=True)


class BowKeys:
    """A frame's or a key frame's keys with its DBoW2::FeatureVector, and the vieo_bow_keys record (arrays kept alive
    here).  feat_vec: list of (node id, [feature indices]) in ascending node order.  mp_id (key frames): per key the id
    of its map point, -1 for none or a bad one."""

    def __init__(self, keys, descriptors, feat_vec, mp_id=None):
        from .orb_extractor import KEYPOINT_DTYPE
        self.keys = np.ascontiguousarray(keys, KEYPOINT_DTYPE)
        self.desc = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
        self.feat_vec = [(int(n), [int(i) for i in f]) for n, f in feat_vec]
        self.mp_id = None if mp_id is None else np.ascontiguousarray(mp_id, np.int32)
        self.node_id = np.array([n for n, _ in self.feat_vec], np.uint32)
        self.node_first = np.zeros(len(self.feat_vec) + 1, np.int32)
        self.node_first[1:] = np.cumsum([len(f) for _, f in self.feat_vec])
        self.node_feat = np.array([i for _, f in self.feat_vec for i in f], np.int32)
        r = np.zeros(1, BOW_KEYS_DTYPE)
        r["n_keys"], r["n_nodes"] = len(self.keys), len(self.node_id)
        for name, arr in (("keys", self.keys), ("descriptors", self.desc), ("mp_id", self.mp_id), ("node_id", self.node_id),
                          ("node_first", self.node_first), ("node_feat", self.node_feat)):
            if arr is not None and arr.size:
                r[name] = arr.ctypes.data
        self.rec = r

    @classmethod
    def from_transform(cls, keys, descriptors, bow, mp_id=None):
        """with mFeatVec = the node_* arrays of a place_recognition.BowResult, passed on as transform wrote them"""
        self = cls(keys, descriptors, [], mp_id)
        self.place = bow  # (keeps the arrays alive)
        self.node_id, self.node_first, self.node_feat = bow.node_id, bow.node_first, bow.node_feat
        self.feat_vec = bow.feat_vec()
        self.rec["n_nodes"] = len(bow.node_id)
        if len(bow.node_id):
            self.rec["node_id"], self.rec["node_first"] = bow.node_id.ctypes.data, bow.node_first.ctypes.data
            self.rec["node_feat"] = bow.node_feat.ctypes.data
        return self


def SearchByBoW(key_frames, frame, mfNNratio=0.6, mbCheckOrientation=True):
    """int ORBmatcher::SearchByBoW(pKF, F, vpMapPointMatches) of every key frame of the list against the frame, in one
    call.  returns [(match int32[F.N] -- the key-frame key whose map point vpMapPointMatches[i] holds, -1 none --, the
    reference's return value)] per key frame."""
    recs = np.concatenate([k.rec for k in key_frames])
    n = len(frame.keys)
    match = np.full((len(key_frames), max(n, 1)), -1, np.int32)
    n_matches = np.zeros(len(key_frames), np.int32)
    rc = _lib.lib().vieo_search_by_bow(frame.rec.ctypes.data, recs.ctypes.data, len(key_frames), float(mfNNratio),
                                       int(bool(mbCheckOrientation)), match.ctypes.data, n_matches.ctypes.data)
    _lib.check(rc, "vieo_search_by_bow")
    return [(match[p, :n].copy(), int(n_matches[p])) for p in range(len(key_frames))]


def SearchByBoWRig(key_frames, frame, key_cam, n_cams, mfNNratio=0.6, mbCheckOrientation=True):
    """SearchByBoW for a frame of a camera rig (F.mapn2in_ filled): key_cam[j] = the image of frame key j, below n_cams.
    Best and second best are kept per image, so a key-frame key can hand its map point to one frame key per camera.
    returns SearchByBoW's list."""
    recs = np.concatenate([k.rec for k in key_frames])
    n = len(frame.keys)
    key_cam = np.ascontiguousarray(key_cam, np.uint8).reshape(-1)
    if len(key_cam) != n:
        raise ValueError("SearchByBoWRig: key_cam differs in length from the frame's keys")
    match = np.full((len(key_frames), max(n, 1)), -1, np.int32)
    n_matches = np.zeros(len(key_frames), np.int32)
    rc = _lib.lib().vieo_search_by_bow_rig(frame.rec.ctypes.data, key_cam.ctypes.data if n else None, int(n_cams),
                                           recs.ctypes.data, len(key_frames), float(mfNNratio), int(bool(mbCheckOrientation)),
                                           match.ctypes.data, n_matches.ctypes.data)
    _lib.check(rc, "vieo_search_by_bow_rig")
    return [(match[p, :n].copy(), int(n_matches[p])) for p in range(len(key_frames))]


def make_bow_rig_scene(seed, n_cams, n_kfs=3, n_keys=300, n_nodes=40):
    """make_bow_scene for a rig frame: the frame's keys are camera-major (key_cam ascending) over n_cams images, one of
    which -- the last but one when there are three or more, else none -- has no keys at all.  About a third of the
    key-frame keys that view a frame key get further views in other images (the frame key's descriptor with a few
    bits flipped, the same node), two or three images in all, and some frame keys are equally good for two key-frame
    keys.  returns (BowKeys frame, key_cam uint8, cam_first int32[n_cams + 1], [BowKeys key frames])."""
    frame, kfs = make_bow_scene(seed, n_kfs, n_keys, n_nodes)
    rng = np.random.default_rng([seed, 77])
    used = [c for c in range(n_cams) if not (n_cams >= 3 and c == n_cams - 2)]
    key_cam = np.sort(np.array(used, np.uint8)[rng.integers(0, len(used), n_keys)])
    cam_first = np.searchsorted(key_cam, np.arange(n_cams + 1)).astype(np.int32)
    cam_first[n_cams] = n_keys
    if len(used) < 2:
        return frame, key_cam, cam_first, kfs
    # further views: frame key b2 (another image) repeats frame key b (descriptor, node, angle), so that the key-frame
    # keys that view b find a best match in b2's image as well
    f_desc, f_keys = frame.desc.copy(), frame.keys.copy()
    node_of = np.zeros(n_keys, np.int64)
    for nd, idx in frame.feat_vec:
        node_of[idx] = nd
    free = set(range(n_keys // 5, n_keys))  # (the near-duplicates of make_bow_scene stay as they are)
    for b in rng.choice(np.arange(n_keys // 5, n_keys), n_keys // 6, replace=False):
        b = int(b)
        if b not in free:
            continue
        free.discard(b)
        others = [c for c in used if c != key_cam[b]]
        rng.shuffle(others)
        for c in others[:int(rng.integers(1, 3))]:
            pool = [j for j in free if key_cam[j] == c]
            if not pool:
                continue
            b2 = int(pool[int(rng.integers(0, len(pool)))])
            free.discard(b2)
            d = f_desc[b].copy()
            for bit in rng.choice(256, int(rng.integers(0, 6)), replace=False):
                d[bit // 8] ^= np.uint8(1 << (bit % 8))
            f_desc[b2], node_of[b2] = d, node_of[b]
            f_keys["angle"][b2] = f_keys["angle"][b]
    fv = [(int(nd), [int(i) for i in np.flatnonzero(node_of == nd)]) for nd in np.unique(node_of)]
    # a frame key equally good for two key-frame keys: key b of the key frame becomes an exact copy of key a (another
    # map point), so whichever comes first in the node takes the frame key and the other finds it taken
    out = []
    for kf in kfs:
        k_desc, k_keys, k_node = kf.desc.copy(), kf.keys.copy(), np.zeros(len(kf.keys), np.int64)
        for nd, idx in kf.feat_vec:
            k_node[idx] = nd
        held = np.flatnonzero(kf.mp_id >= 0)
        for a, b in rng.choice(held, (6, 2), replace=False):
            k_desc[b], k_node[b], k_keys["angle"][b] = k_desc[a], k_node[a], k_keys["angle"][a]
        kfv = [(int(nd), [int(i) for i in np.flatnonzero(k_node == nd)]) for nd in np.unique(k_node)]
        out.append(BowKeys(k_keys, k_desc, kfv, kf.mp_id))
    return BowKeys(f_keys, f_desc, fv), key_cam, cam_first, out


def make_bow_scene(seed, n_kfs=3, n_keys=300, n_nodes=40):
    """A frame and n_kfs key frames for SearchByBoW: n_keys keys each in about n_nodes vocabulary nodes.  About 60 % of a
    key frame's keys are views of frame keys (a few descriptor bits flipped, the same node, the frame's angle plus the
    key frame's rotation); planted on top: frame keys with a near-duplicate in their node (the ratio test rejects),
    key-frame keys that copy another one's descriptor (the frame key is taken when their turn comes), map points seen
    by two keys of a key frame (the (map point, image) table replaces or keeps), and views with a random angle (the
    rotation histogram removes them).  returns (BowKeys frame, [BowKeys key frames])."""
    from .orb_extractor import KEYPOINT_DTYPE
    rng = np.random.default_rng(seed)
    node_ids = np.sort(rng.choice(100000, n_nodes + 8, replace=False)).astype(np.uint32)
    shared = node_ids[:n_nodes]

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

    f_desc = rng.integers(0, 256, (n_keys, 32), dtype=np.uint8)
    f_node = shared[rng.integers(0, n_nodes, n_keys)]
    f_angle = rng.uniform(0, 360, n_keys).astype(np.float32)
    for i in range(0, n_keys // 10):  # near-duplicates inside the frame: key 2i+1 repeats key 2i
        f_desc[2 * i + 1], f_node[2 * i + 1] = flip(f_desc[2 * i], 3), f_node[2 * i]
    frame = BowKeys(keys_of(f_angle), f_desc, feat_vec(f_node))
    kfs = []
    for p in range(n_kfs):
        rot = rng.uniform(0, 360)
        k_desc = rng.integers(0, 256, (n_keys, 32), dtype=np.uint8)
        own = np.concatenate([shared[p::2], node_ids[n_nodes + 2 * p:n_nodes + 2 * p + 4]])  # half the shared nodes + own ones
        k_node = own[rng.integers(0, len(own), n_keys)]
        k_angle = rng.uniform(0, 360, n_keys).astype(np.float32)
        mp = np.where(rng.uniform(size=n_keys) < 0.75, np.arange(n_keys) + 1000 * p, -1).astype(np.int32)
        views = rng.choice(n_keys, int(0.6 * n_keys), replace=False)
        src = rng.choice(n_keys, len(views), replace=False)
        for j, (a, b) in enumerate(zip(views, src)):
            k_desc[a], k_node[a] = flip(f_desc[b], int(rng.integers(0, 40))), f_node[b]
            ang = f_angle[b] + rot + rng.normal(0, 2.0) if j % 8 else rng.uniform(0, 360)
            k_angle[a] = np.float32(ang % 360.0)
        for j in range(0, 40, 2):  # a second key-frame key on the same frame key, with another map point
            a, b = views[j], views[j + 1]
            k_desc[b], k_node[b], k_angle[b] = flip(k_desc[a], 2), k_node[a], k_angle[a]
        for j in range(40, 90, 2):  # two keys of the key frame hold the same map point
            a, b = views[j], views[j + 1]
            if mp[a] >= 0:
                mp[b] = mp[a]
        k_angle[k_angle >= 360.0] = 0.0
        kfs.append(BowKeys(keys_of(k_angle), k_desc, feat_vec(k_node), mp))
    return frame, kfs


# ---------------------------------------------------------------------------------------------------------------------
# the chain: Tracking::Relocalization
RELOC_FRAME_DTYPE = np.dtype([("n_keys", np.int32), ("n_levels", np.int32), ("keys", np.uint64), ("uright", np.uint64),
                              ("descriptors", np.uint64), ("level_sigma2", np.uint64), ("inv_level_sigma2", np.uint64),
                              ("scale_factor", np.uint64), ("log_scale_factor", np.float32), ("fx", np.float32),
                              ("fy", np.float32), ("cx", np.float32), ("cy", np.float32), ("bf", np.float32),
                              ("bounds", np.float32, 4), ("n_nodes", np.int32), ("n_cams", np.int32),
                              ("Rcb", np.float64, 9), ("tcb", np.float64, 3), ("node_id", np.uint64),
                              ("node_first", np.uint64), ("node_feat", np.uint64)], align=True)
RELOC_CANDIDATE_DTYPE = np.dtype([("kf", BOW_KEYS_DTYPE), ("points", np.uint64)], align=True)
RELOC_VISIT_DTYPE = np.dtype([("cand", np.int32), ("call", np.int32), ("row", np.int32), ("no_more", np.int32),
                              ("found", np.int32), ("n_inliers", np.int32), ("n_good", np.int32, 3),
                              ("n_additional", np.int32, 2), ("reserved", np.int32)], align=True)


def _reloc_result_dtype():
    from .ba_types import NAVSTATE_DTYPE
    return np.dtype([("found", np.int32), ("cand", np.int32), ("n_good", np.int32), ("n_visits", np.int32),
                     ("nav", NAVSTATE_DTYPE), ("Tcw", np.float32, 16)], align=True)


RELOC_RESULT_DTYPE = _reloc_result_dtype()


def nav_from_tcw(Tcw, Rcb, tcb):
    """Frame::UpdateNavStatePVRFromTcw: (pwb, qwb (w, x, y, z)) of Twb = (Tbc * Tcw)^-1, in double from the float Tcw"""
    T = np.asarray(Tcw, np.float32).astype(np.float64).reshape(4, 4)
    Rcb, tcb = np.asarray(Rcb, np.float64).reshape(3, 3), np.asarray(tcb, np.float64)
    Rbw = Rcb.T @ T[:3, :3]
    tbw = Rcb.T @ T[:3, 3] - Rcb.T @ tcb
    R = Rbw.T
    p = -(R @ tbw)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = math.sqrt(tr + 1.0) * 2
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = math.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2
        q = [(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif R[1, 1] > R[2, 2]:
        s = math.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s]
    else:
        s = math.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s]
    q = np.array(q)
    return p, q / np.linalg.norm(q)


def tcw_from_nav(p, q, Rcb, tcb):
    """Frame::UpdatePoseFromNS: the float 4 x 4 Tcw = Tcb * Twb^-1"""
    w, x, y, z = (float(v) for v in q)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    Rcb, tcb = np.asarray(Rcb, np.float64).reshape(3, 3), np.asarray(tcb, np.float64)
    pwc = R @ (-(Rcb.T @ tcb)) + np.asarray(p, np.float64)
    Rcw = Rcb @ R.T
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = Rcw.astype(np.float32), (-(Rcw @ pwc)).astype(np.float32)
    return T


class RelocFrame:
    """The lost frame: mvKeysUn, uright, descriptors, mFeatVec, the pyramid's tables, intrinsics and Tcb (arrays kept
    alive here) and its vieo_reloc_frame record.  A frame of a Tracker enters through the keys / desc / uright of its
    output."""

    def __init__(self, keys, uright, descriptors, feat_vec, K, bf, scale_factor, bounds=(0, WIDTH, 0, HEIGHT),
                 Rcb=np.eye(3), tcb=np.zeros(3), n_cams=0):
        self.bow = BowKeys(keys, descriptors, feat_vec)
        self.keys, self.desc = self.bow.keys, self.bow.desc
        self.uright = np.ascontiguousarray(uright, np.float32)
        self.scale = np.ascontiguousarray(scale_factor, np.float32)
        self.sigma2 = (self.scale * self.scale).astype(np.float32)
        self.inv_sigma2 = (np.float32(1.0) / self.sigma2).astype(np.float32)
        self.log_scale = float(np.float32(math.log(float(self.scale[1] if len(self.scale) > 1 else 1.2))))
        self.K, self.bf = tuple(float(np.float32(k)) for k in K), float(np.float32(bf))
        self.bounds = np.asarray(bounds, np.float32)
        self.Rcb, self.tcb = np.asarray(Rcb, np.float64).reshape(3, 3), np.asarray(tcb, np.float64)
        r = np.zeros(1, RELOC_FRAME_DTYPE)
        r["n_keys"], r["n_levels"], r["n_nodes"], r["n_cams"] = len(self.keys), len(self.scale), len(self.bow.node_id), n_cams
        for name, arr in (("keys", self.keys), ("uright", self.uright), ("descriptors", self.desc),
                          ("level_sigma2", self.sigma2), ("inv_level_sigma2", self.inv_sigma2), ("scale_factor", self.scale),
                          ("node_id", self.bow.node_id), ("node_first", self.bow.node_first), ("node_feat", self.bow.node_feat)):
            if arr.size:
                r[name] = arr.ctypes.data
        r["log_scale_factor"], r["bf"] = self.log_scale, self.bf
        r["fx"], r["fy"], r["cx"], r["cy"] = self.K
        r["bounds"], r["Rcb"], r["tcb"] = self.bounds, self.Rcb.reshape(-1), self.tcb
        self.rec = r


class RelocCandidate:
    """A candidate key frame: its BowKeys and GetMapPointMatches() flattened (KEYFRAME_POINT_DTYPE per key)."""

    def __init__(self, bow, points):
        from .ba_types import KEYFRAME_POINT_DTYPE
        self.bow = bow
        self.points = np.ascontiguousarray(points, KEYFRAME_POINT_DTYPE)
        assert len(self.points) == len(bow.keys)
        r = np.zeros(1, RELOC_CANDIDATE_DTYPE)
        r["kf"] = bow.rec[0]
        r["points"] = self.points.ctypes.data
        self.rec = r


def relocalize_call(frame, candidates, samples=None, n_rows=None, seed=0, trace_capacity=256):
    """vieo_relocalize, raw: (rc, result record, mp_ref, outlier, trace)"""
    recs = np.concatenate([c.rec for c in candidates])
    if samples is not None:
        samples = np.ascontiguousarray(np.stack([np.asarray(s, np.int32).reshape(-1, 4) for s in samples]))
        n_rows = samples.shape[1]
    n = len(frame.keys)
    res = np.zeros(1, RELOC_RESULT_DTYPE)
    mp_ref, outlier = np.full(max(n, 1), -7, np.int32), np.full(max(n, 1), 7, np.uint8)
    trace = np.zeros(trace_capacity, RELOC_VISIT_DTYPE)
    rc = _lib.lib().vieo_relocalize(frame.rec.ctypes.data, recs.ctypes.data, len(candidates),
                                    samples.ctypes.data if samples is not None else None, int(n_rows), int(seed),
                                    res.ctypes.data, mp_ref.ctypes.data, outlier.ctypes.data, trace.ctypes.data, trace_capacity)
    return rc, res[0], mp_ref[:n], outlier[:n], trace


def Relocalization(frame, candidates, samples=None, n_rows=320, seed=0):
    """bool Tracking::Relocalization() for the frame against the candidate key frames (Tracking.cc:2541-2663).
    returns dict(found, cand, n_good, Tcw (4, 4) float32, nav, mp_ref, outlier, trace)."""
    rc, res, mp_ref, outlier, trace = relocalize_call(frame, candidates, samples, n_rows, seed)
    _lib.check(rc, "vieo_relocalize")
    return dict(found=bool(res["found"]), cand=int(res["cand"]), n_good=int(res["n_good"]),
                Tcw=res["Tcw"].reshape(4, 4).copy(), nav=res["nav"].copy(), mp_ref=mp_ref, outlier=outlier.astype(bool),
                trace=trace[:int(res["n_visits"])].copy())


class RelocRig:
    """The cameras of a rig frame for RelocalizationRig, and the vieo_reloc_rig record (arrays kept alive here): pnp =
    PNP_RIG_DTYPE[1] (make_pnp_rig), cam_first int32[n_cams + 1] over the frame's camera-major keys (mapn2in_), sbp =
    SBP_RIG_DTYPE[1] (synth_fisheye.make_sbp_rig), pose_cams = CAMERA_DTYPE[n_cams] with Rcb / tcb composed (what
    vieo_pose_frame.cams takes)."""

    def __init__(self, pnp, cam_first, sbp, pose_cams):
        from .ba_types import CAMERA_DTYPE, SBP_RIG_DTYPE
        self.pnp = np.ascontiguousarray(pnp, PNP_RIG_DTYPE).reshape(1)
        self.cam_first = np.ascontiguousarray(cam_first, np.int32).reshape(-1)
        self.sbp = None if sbp is None else np.ascontiguousarray(sbp, SBP_RIG_DTYPE).reshape(1)
        self.pose_cams = np.ascontiguousarray(pose_cams, CAMERA_DTYPE).reshape(-1)
        self.n_cams = int(self.pnp["n_cams"][0])
        r = np.zeros(1, RELOC_RIG_DTYPE)
        r["pnp"] = self.pnp[0]
        r["cam_first"], r["pose_cams"] = self.cam_first.ctypes.data, self.pose_cams.ctypes.data
        r["sbp"] = 0 if self.sbp is None else self.sbp.ctypes.data
        self.rec = r

    def key_cam(self):
        """get<0>(mapn2in_[j]) of every frame key"""
        return np.repeat(np.arange(len(self.cam_first) - 1), np.diff(self.cam_first)).astype(np.uint8)


def relocalize_rig_call(frame, rig, candidates, samples=None, n_rows=None, seed=0, trace_capacity=256):
    """vieo_relocalize_rig, raw: (rc, result record, mp_ref, outlier, trace)"""
    recs = np.concatenate([c.rec for c in candidates])
    if samples is not None:
        samples = np.ascontiguousarray(np.stack([np.asarray(s, np.int32).reshape(-1, 4) for s in samples]))
        n_rows = samples.shape[1]
    n = len(frame.keys)
    res = np.zeros(1, RELOC_RESULT_DTYPE)
    mp_ref, outlier = np.full(max(n, 1), -7, np.int32), np.full(max(n, 1), 7, np.uint8)
    trace = np.zeros(trace_capacity, RELOC_VISIT_DTYPE)
    rc = _lib.lib().vieo_relocalize_rig(frame.rec.ctypes.data, rig.rec.ctypes.data, recs.ctypes.data, len(candidates),
                                        samples.ctypes.data if samples is not None else None, int(n_rows), int(seed),
                                        res.ctypes.data, mp_ref.ctypes.data, outlier.ctypes.data, trace.ctypes.data,
                                        trace_capacity)
    return rc, res[0], mp_ref[:n], outlier[:n], trace


def RelocalizationRig(frame, rig, candidates, samples=None, n_rows=320, seed=0):
    """Tracking::Relocalization for a frame of a camera rig (Frame::usedistort_): frame = a RelocFrame with keys = mvKeys
    in camera-major order, n_cams = the rig's, K = camera 0's toK(), Rcb / tcb = body -> reference camera; rig = a
    RelocRig.  returns Relocalization's dict."""
    rc, res, mp_ref, outlier, trace = relocalize_rig_call(frame, rig, candidates, samples, n_rows, seed)
    _lib.check(rc, "vieo_relocalize_rig")
    return dict(found=bool(res["found"]), cand=int(res["cand"]), n_good=int(res["n_good"]),
                Tcw=res["Tcw"].reshape(4, 4).copy(), nav=res["nav"].copy(), mp_ref=mp_ref, outlier=outlier.astype(bool),
                trace=trace[:int(res["n_visits"])].copy())


def RelocalizationFromPlaceRecognition(bow, candidate_ids, key_frames, keys, uright, descriptors, K, bf, scale_factor,
                                       samples=None, n_rows=320, seed=0, rig=None, **frame_args):
    """Tracking::Relocalization with the vocabulary's part on the device as well: `bow` is the frame's
    place_recognition.BowResult (transform, i.e. ComputeBoW), `candidate_ids` what KeyFrameDatabase.detect_reloc
    returned for bow.word_id / bow.word_value, `key_frames` maps a key-frame id to its RelocCandidate.  The frame's
    mFeatVec arrays go into the vieo_reloc_frame record as transform wrote them.  Without candidates the reference
    returns false before anything else (Tracking.cc:2534); so does this.  rig: a RelocRig for a frame of a camera rig
    (keys = mvKeys, camera-major; K = camera 0's toK()).  returns Relocalization's dict."""
    if rig is not None:
        frame_args = dict(frame_args, n_cams=rig.n_cams)
    frame = RelocFrame(keys, uright, descriptors, [], K, bf, scale_factor, **frame_args)
    frame.place = bow  # (keeps the arrays alive)
    frame.rec["n_nodes"] = len(bow.node_id)
    if len(bow.node_id):
        frame.rec["node_id"], frame.rec["node_first"] = bow.node_id.ctypes.data, bow.node_first.ctypes.data
        frame.rec["node_feat"] = bow.node_feat.ctypes.data
    cands = [key_frames[int(i)] for i in candidate_ids]
    if not cands:
        n = len(frame.keys)
        return dict(found=False, cand=-1, n_good=0, Tcw=np.eye(4, dtype=np.float32), nav=None, mp_ref=np.full(n, -1, np.int32),
                    outlier=np.zeros(n, bool), trace=np.zeros(0, RELOC_VISIT_DTYPE))
    if rig is not None:
        return RelocalizationRig(frame, rig, cands, samples, n_rows, seed)
    return Relocalization(frame, cands, samples, n_rows, seed)


def make_reloc_scene(seed, kind="widen"):
    """A lost frame and its relocalisation candidates.  kind:
      "widen"   candidate 0 is true with 45 true + 8 false BoW matches and 120 more of its map points in view (the
                th = 10 search has to find them); candidate 1 has 5 matches (discarded); candidate 2 has 20 matches whose
                map points lie anywhere (ends in bNoMore)
      "direct"  candidate 0 is true with 120 true + 15 false BoW matches
      "none"    no true candidate: one with 5 matches, two with 20 random ones
      "narrow"  candidate 0 is true with 33 true + 4 false BoW matches, 9 more map points in view and 8 frame keys that look
                like further map points but lie 6 px away: after the th = 10 search the optimisation lands between 30 and 50
    returns (RelocFrame, [RelocCandidate], dict(R, t) -- the true pose Tcw)."""
    from .ba_types import KEYFRAME_POINT_DTYPE
    from .orb_extractor import KEYPOINT_DTYPE
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = CAMERA_K
    n_levels = 8
    scale = (np.float32(1.2) ** np.arange(n_levels)).astype(np.float32)
    R, t = rodrigues(rng.standard_normal(3) * 0.15), rng.standard_normal(3) * 0.3
    Ow = -R.T @ t
    plan = {"widen": [(45, 8, 120, 0), (5, 0, 0, 0), (0, 20, 0, 0)], "direct": [(120, 15, 0, 0)],
            "none": [(0, 5, 0, 0), (0, 20, 0, 0), (0, 20, 0, 0)], "narrow": [(33, 4, 9, 8)]}[kind]
    node = [1000]
    f_keys, f_desc, f_node = [], [], []
    cands = []

    def new_node():
        node[0] += int(rng.integers(1, 9))
        return node[0]

    def flip(desc, nbits):
        d = desc.copy()
        for b in rng.choice(256, nbits, replace=False):
            d[b // 8] ^= np.uint8(1 << (b % 8))
        return d

    def frame_key(u, v, octave, angle, desc, nd):
        k = np.zeros(1, KEYPOINT_DTYPE)
        k["x"], k["y"], k["size"], k["angle"], k["octave"] = u, v, 31.0, angle % 360.0, octave
        f_keys.append(k)
        f_desc.append(desc)
        f_node.append(nd)

    for n_true, n_false, n_more, n_near in plan:
        n = n_true + n_false + n_more + n_near
        rot = rng.uniform(0, 360)
        u, v, z = rng.uniform(40, WIDTH - 40, n), rng.uniform(40, HEIGHT - 40, n), rng.uniform(1.5, 12.0, n)
        Pc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], axis=1)
        Xw = ((Pc - t) @ R).astype(np.float32)
        octave = rng.integers(0, 4, n)
        pts = np.zeros(n, KEYFRAME_POINT_DTYPE)
        kk = np.zeros(n, KEYPOINT_DTYPE)
        kdesc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        kk["x"], kk["y"] = rng.uniform(20, WIDTH - 20, n), rng.uniform(20, HEIGHT - 20, n)
        kk["size"], kk["angle"], kk["octave"] = 31.0, rng.uniform(0, 359, n).astype(np.float32), octave
        dist = np.linalg.norm(Xw.astype(np.float64) - Ow, axis=1)
        pts["Xw"], pts["octave"], pts["angle"], pts["flags"], pts["desc"] = Xw, octave, kk["angle"], 3, kdesc
        pts["max_distance"] = dist * 1.2 ** (octave - 0.5)
        pts["min_distance"] = pts["max_distance"] / np.float32(1.2 ** (n_levels - 1))
        k_node = np.zeros(n, np.int64)
        for i in range(n):
            noise = rng.standard_normal(2) * 0.5 * float(scale[octave[i]])
            ang = float(kk["angle"][i]) + rot + rng.normal(0, 1.0)
            if i < n_true:  # a BoW match at the point's projection
                k_node[i] = new_node()
                frame_key(u[i] + noise[0], v[i] + noise[1], octave[i], ang, flip(kdesc[i], int(rng.integers(0, 12))), k_node[i])
            elif i < n_true + n_false:  # a BoW match anywhere in the image
                k_node[i] = new_node()
                frame_key(rng.uniform(20, WIDTH - 20), rng.uniform(20, HEIGHT - 20), octave[i], ang,
                          flip(kdesc[i], int(rng.integers(0, 12))), k_node[i])
            elif i < n_true + n_false + n_more:  # in view, but the vocabulary puts the two keys into different nodes
                k_node[i] = new_node()
                frame_key(u[i] + noise[0], v[i] + noise[1], octave[i], ang, flip(kdesc[i], int(rng.integers(0, 30))), new_node())
            else:  # looks like the point, lies 6 px (times its level's scale) beside the projection
                k_node[i] = new_node()
                d = rng.standard_normal(2)
                d = d / np.linalg.norm(d) * 6.0 * float(scale[octave[i]])
                frame_key(u[i] + d[0], v[i] + d[1], octave[i], ang, flip(kdesc[i], int(rng.integers(0, 30))), new_node())
        fv = sorted((int(nd), [i]) for i, nd in enumerate(k_node))
        cands.append(RelocCandidate(BowKeys(kk, kdesc, fv, np.arange(n, dtype=np.int32) + 10000 * len(cands)), pts))
    order = rng.permutation(len(f_keys))
    keys = np.concatenate(f_keys)[order]
    keys["angle"][keys["angle"] >= 360.0] = 0.0  # (the float32 rounding of a value just below 360)
    desc = np.stack(f_desc)[order]
    nodes = np.array(f_node)[order]
    fv = sorted((int(nd), [i]) for i, nd in enumerate(nodes))
    frame = RelocFrame(keys, np.full(len(keys), -1.0, np.float32), desc, fv, CAMERA_K, 47.9, scale)
    return frame, cands, dict(R=R, t=t)


def make_reloc_rig_scene(seed, kind="widen", rig_kind="radtan2", plane_z=None):
    """make_reloc_scene for a lost frame of a camera rig (kinds "widen", "direct", "none" with the same plans): every
    map point lies in the view of camera i % n_cams and its frame key is that camera model's projection; every fourth
    true BoW match has a second frame key in another camera that sees the point (the same node, the point's descriptor
    again), so the map point is matched in two images.  The frame's keys are mvKeys in camera-major order, uright -1.
    plane_z: as for make_pnp_rig_scene.
    returns (RelocFrame, RelocRig, [RelocCandidate], dict(R, t) -- the true pose of the reference camera)."""
    from . import synth_ba
    from .ba_types import KEYFRAME_POINT_DTYPE
    from .orb_extractor import KEYPOINT_DTYPE
    from .synth_fisheye import make_sbp_rig
    rng = np.random.default_rng(seed)
    rig = rig_of(rig_kind)
    nc = len(rig["cams"])
    W, H = rig["size"]
    n_levels = 8
    scale = (np.float32(1.2) ** np.arange(n_levels)).astype(np.float32)
    R, t = rodrigues(rng.standard_normal(3) * 0.15), rng.standard_normal(3) * 0.3
    Ow = -R.T @ t
    plan = {"widen": [(36, 8, 120)], "direct": [(120, 15, 0)], "none": [(0, 5, 0), (0, 20, 0), (0, 20, 0)]}[kind]  # (36 + 9 second views)
    if kind == "widen":
        plan += [(5, 0, 0), (0, 20, 0)]
    node = [1000]
    f_keys, f_desc, f_node, f_cam = [], [], [], []
    cands = []

    def new_node():
        node[0] += int(rng.integers(1, 9))
        return node[0]

    def flip(desc, nbits):
        d = desc.copy()
        for b in rng.choice(256, nbits, replace=False):
            d[b // 8] ^= np.uint8(1 << (b % 8))
        return d

    def frame_key(c, u, v, octave, angle, desc, nd):
        k = np.zeros(1, KEYPOINT_DTYPE)
        k["x"], k["y"], k["size"], k["angle"], k["octave"] = u, v, 31.0, angle % 360.0, octave
        f_keys.append(k), f_desc.append(desc), f_node.append(nd), f_cam.append(c)

    for n_true, n_false, n_more in plan:
        n = n_true + n_false + n_more
        rot = rng.uniform(0, 360)
        Pr, px, cam = np.zeros((n, 3)), np.zeros((n, 2)), np.arange(n) % nc
        for i in range(n):
            Pr[i], px[i] = _draw_rig_point(rng, rig, int(cam[i]), plane_z, 40.0)
        Xw = ((Pr - t) @ R).astype(np.float32)
        octave = rng.integers(0, 4, n)
        pts = np.zeros(n, KEYFRAME_POINT_DTYPE)
        kk = np.zeros(n, KEYPOINT_DTYPE)
        kdesc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        kk["x"], kk["y"] = rng.uniform(20, W - 20, n), rng.uniform(20, H - 20, n)
        kk["size"], kk["angle"], kk["octave"] = 31.0, rng.uniform(0, 359, n).astype(np.float32), octave
        dist = np.linalg.norm(Xw.astype(np.float64) - Ow, axis=1)
        pts["Xw"], pts["octave"], pts["angle"], pts["flags"], pts["desc"] = Xw, octave, kk["angle"], 3, kdesc
        pts["max_distance"] = dist * 1.2 ** (octave - 0.5)
        pts["min_distance"] = pts["max_distance"] / np.float32(1.2 ** (n_levels - 1))
        k_node = np.zeros(n, np.int64)
        for i in range(n):
            noise = rng.standard_normal(2) * 0.5 * float(scale[octave[i]])
            ang = float(kk["angle"][i]) + rot + rng.normal(0, 1.0)
            k_node[i] = new_node()
            if i < n_true:  # a BoW match at the point's projection
                frame_key(cam[i], px[i, 0] + noise[0], px[i, 1] + noise[1], octave[i], ang,
                          flip(kdesc[i], int(rng.integers(0, 12))), k_node[i])
                if i % 4 == 0:  # and a second one in another camera that sees the point
                    for c in list(range(cam[i] + 1, nc)) + list(range(cam[i])):
                        uv = _rig_view(rig, c, Pr[i], 40.0)
                        if uv is not None:
                            noise = rng.standard_normal(2) * 0.5 * float(scale[octave[i]])
                            frame_key(c, uv[0] + noise[0], uv[1] + noise[1], octave[i], ang,
                                      flip(kdesc[i], int(rng.integers(0, 12))), k_node[i])
                            break
            elif i < n_true + n_false:  # a BoW match anywhere in the image
                frame_key(cam[i], rng.uniform(20, W - 20), rng.uniform(20, H - 20), octave[i], ang,
                          flip(kdesc[i], int(rng.integers(0, 12))), k_node[i])
            else:  # in view, but the vocabulary puts the two keys into different nodes
                frame_key(cam[i], px[i, 0] + noise[0], px[i, 1] + noise[1], octave[i], ang,
                          flip(kdesc[i], int(rng.integers(0, 30))), new_node())
        fv = sorted((int(nd), [i]) for i, nd in enumerate(k_node))
        cands.append(RelocCandidate(BowKeys(kk, kdesc, fv, np.arange(n, dtype=np.int32) + 10000 * len(cands)), pts))
    f_cam = np.array(f_cam)
    order = rng.permutation(len(f_keys))
    order = order[np.argsort(f_cam[order], kind="stable")]  # mvKeys: camera-major
    keys = np.concatenate(f_keys)[order]
    keys["angle"][keys["angle"] >= 360.0] = 0.0  # (the float32 rounding of a value just below 360)
    desc = np.stack(f_desc)[order]
    nodes = np.array(f_node)[order]
    by_node = {}
    for i, nd in enumerate(nodes):
        by_node.setdefault(int(nd), []).append(i)
    fv = sorted(by_node.items())
    cam_first = np.searchsorted(f_cam[order], np.arange(nc + 1)).astype(np.int32)
    Tcb = np.linalg.inv(synth_ba.EUROC_TBC)  # body -> reference camera, what camera_rig composed into the cameras' Rcb / tcb
    bounds = np.tile(np.array([0, W, 0, H], np.float32), (nc, 1))
    frame = RelocFrame(keys, np.full(len(keys), -1.0, np.float32), desc, fv, rig["K"], 0.11 * rig["K"][0], scale,
                       bounds=bounds[0], Rcb=Tcb[:3, :3], tcb=Tcb[:3, 3], n_cams=nc)
    rr = RelocRig(rig["pnp"], cam_first, make_sbp_rig(rig["cams"], rig["Tcr"], bounds, True), rig["cams"])
    return frame, rr, cands, dict(R=R, t=t)
