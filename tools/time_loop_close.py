"""Times the two projection searches of a loop closure that take a Sim3 world pose, on one scene per camera count
(one rectified camera, the 4-camera KB8 rig): 32 corrected key frames of 1200 keys -- the candidates of
loop_closing.make_loop_pair_scene, which all look at the same neighbourhood -- and 4000 loop points, the first 4000 map
points of those key frames.
  - vieo_fuse_scw: Fuse(pKF, Scw, ...) of all 32 key frames in ONE call, against the only way to run the same search
    without it: vieo_fuse_search once per key frame on the same transforms and masks (built outside the clock, so the
    loop is charged for its calls alone);
  - vieo_search_by_projection_scw of the 4000 points into one key frame;
  - the share of (visit, point, camera) items that pass the gates, which is a property of this scene;
  - vieo_compute_sim3 (SearchByBoW, the Sim3 RANSAC tables, the round-robin with SearchBySim3 and OptimizeSim3) of a key frame
    of 1200 keys against 8 candidates of loop_closing.make_compute_sim3_scene, the library drawing its own samples.
Per figure: a warm-up call, then --repeat calls on a host clock; median (min ... max).  Reports, not thresholds.
Usage: python tools/time_loop_close.py [--repeat 20] [--kfs 32] [--keys 1200] [--points 4000]"""
import argparse
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vieo_slam_amd import _lib  # noqa: E402
from vieo_slam_amd import loop_closing as lc  # noqa: E402
from vieo_slam_amd import map_point as mp  # noqa: E402


def timed_ms(fn, repeat):
    fn()
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def fuse_frame(kf, Scw, th):
    """the vieo_fuse_frame of Fuse(pKF, Scw, ...): the cv::Mat decomposition the header states, the viewing cone on"""
    S = np.asarray(Scw, np.float32).reshape(3, 4)
    dot = (float(S[0, 0]) * float(S[0, 0]) + float(S[0, 1]) * float(S[0, 1])) + float(S[0, 2]) * float(S[0, 2])
    inv = 1.0 / float(np.float32(math.sqrt(dot)))
    FF = np.zeros(1, mp.FUSE_FRAME_DTYPE)
    f = FF[0]["base"]
    f["Rcrw"] = (S[:, :3].astype(np.float64) * inv).astype(np.float32).reshape(-1)
    f["tcrw"], f["Ow"] = (S[:, 3].astype(np.float64) * inv).astype(np.float32), kf.Ow
    f["n_cams"], f["use_distort"], f["cams"] = kf.n_cams, kf.use_distort, kf.cams.ctypes.data
    f["Tcr"][:kf.n_cams], f["trc"][:kf.n_cams], f["bounds"][:kf.n_cams] = kf.Tcr, kf.trc, kf.bounds
    f["log_scale_factor"], f["n_levels"] = kf.log_scale_factor, kf.n_levels
    FF[0]["scale_factors"][:kf.n_levels] = kf.scale_factors
    FF[0]["inv_level_sigma2"][:kf.n_levels] = kf.inv_level_sigma2
    FF[0]["th_radius"], FF[0]["check_viewing_angle"] = th, 1
    return FF


def fuse_mask(kf, ids):
    """vbAlreadyMatched1 as ORBmatcher.cc:1177-1187 writes it"""
    found = set((int(m), int(c)) for m, c in zip(kf.mp_id, kf.cam_of_key) if m >= 0)
    mask = np.zeros(len(ids), np.int32)
    for i in range(len(ids)):
        cam = 0 if len(kf.keys) <= i else int(kf.cam_of_key[i])
        if (int(ids[i]), cam) in found:
            mask[i] = 1 << cam
    return mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--kfs", type=int, default=32)
    ap.add_argument("--keys", type=int, default=1200)
    ap.add_argument("--points", type=int, default=4000)
    a = ap.parse_args()
    if not _lib.lib().vieo_device_available():
        raise SystemExit("no gfx950 device: nothing to time")
    print("runs per figure: %d (median, min ... max) [ms]" % a.repeat)
    for n_cams in (1, 4):
        s = lc.make_loop_pair_scene(500 + n_cams, n_keys=a.keys, n_points=a.keys - 100, n_cams=n_cams, n_cands=a.kfs, rig="kb8")
        kfs = s["kf2s"]
        points, ids, seen = [], [], set()
        for kf in kfs:
            for i in np.flatnonzero(kf.mp_id >= 0):
                if int(kf.mp_id[i]) not in seen and len(ids) < a.points:
                    seen.add(int(kf.mp_id[i]))
                    points.append(kf.points[i].copy())
                    ids.append(int(kf.mp_id[i]))
        points, ids = np.array(points, lc.FUSE_POINT_DTYPE), np.array(ids, np.int32)
        Scws = [(1.0 + 0.001 * c) * np.concatenate([kf.Rcw.astype(np.float64), kf.tcw.astype(np.float64)[:, None]], axis=1)
                for c, kf in enumerate(kfs)]
        visits = [(c, S.astype(np.float32)) for c, S in enumerate(Scws)]
        print("%d camera(s): %d key frames of %d keys, %d loop points" % (n_cams, len(kfs), len(kfs[0].keys), len(ids)))
        # entry B in one call
        one_call = lambda: lc.FuseScw(kfs, points, ids, visits)
        out = one_call()
        items, survivors = lc.scw_gate_stats()
        taps = [lc.fuse_scw_tap(len(ids), n_cams, v) for v in range(len(visits))]
        print("  vieo_fuse_scw, one call               %9.3f (%.3f ... %.3f)   fused per key frame: %d ... %d"
              % (timed_ms(one_call, a.repeat) + (min(o["n_fused"] for o in out), max(o["n_fused"] for o in out))))
        print("  items that pass the gates             %d of %d (%.1f %%)" % (survivors, items, 100.0 * survivors / items))
        # the same search through vieo_fuse_search, one key frame and one camera at a time
        frames, per_cam, pts = [], [], []
        for (c, S), kf in zip(visits, kfs):
            frames.append(fuse_frame(kf, S, lc.TH_SCW_FUSE))
            per_cam.append([np.flatnonzero(kf.cam_of_key == k) for k in range(n_cams)])
            p = points.copy()
            p["skip_mask"] = np.where(points["skip_mask"] < 0, np.int32(-2 ** 31), fuse_mask(kf, ids))
            pts.append(p)
        keys = [[np.ascontiguousarray(kf.keys[k]) for k in pc] for kf, pc in zip(kfs, per_cam)]
        descs = [[np.ascontiguousarray(kf.desc[k]) for k in pc] for kf, pc in zip(kfs, per_cam)]

        def per_key_frame():
            return [mp.fuse_search(frames[v], keys[v], [None] * n_cams, descs[v], pts[v]) for v in range(len(kfs))]

        same = True
        for v, (bi, bd) in enumerate(per_key_frame()):
            bi = bi.copy()
            for k in range(n_cams):
                hit = bi[:, k] >= 0
                bi[hit, k] = per_cam[v][k][bi[hit, k]]
            same = same and np.array_equal(bi, taps[v][0]) and np.array_equal(bd, taps[v][1])
        print("  vieo_fuse_search per key frame        %9.3f (%.3f ... %.3f)   same best keys and distances: %s"
              % (timed_ms(per_key_frame, a.repeat) + (same,)))
        # entry A: the loop points into one key frame
        matched = np.full(len(kfs[0].keys), -1, np.int32)
        search = lambda: lc.SearchByProjectionScw(kfs[:1], points, ids, [(0, visits[0][1], matched)], lc.TH_SCW_SEARCH)
        (_, n), = search()
        items, survivors = lc.scw_gate_stats()
        print("  vieo_search_by_projection_scw         %9.3f (%.3f ... %.3f)   matches: %d, gate: %d of %d"
              % (timed_ms(search, a.repeat) + (n, survivors, items)))
    s = lc.make_compute_sim3_scene(600, n_cands=8, n_keys=a.keys, n_points=a.keys - 100, n_nodes=120)
    chain = lambda: lc.compute_sim3_call(s["kf1"], s["kf2s"], n_rows=300, seed=1)
    rc, o = chain()
    print("ComputeSim3, 8 candidates of %d keys: rc %d, matched candidate %d with %d inliers, %d trace lines"
          % (len(s["kf2s"][0].keys), rc, o["cand"], o["n_inliers"], o["n_visits"]))
    print("  vieo_compute_sim3                     %9.3f (%.3f ... %.3f)" % timed_ms(chain, a.repeat))


if __name__ == "__main__":
    main()
