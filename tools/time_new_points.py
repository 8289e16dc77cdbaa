"""Times the new-map-point entries on the GPU: ms per call of vieo_triangulate_new_points and of
vieo_create_new_map_points, with vieo_search_for_triangulation alone on the same input beside them.

Workloads: 10 undistorted neighbours at n_points = 3000, and the 4-camera KB8 rig with 8 neighbours.  Every call is
synchronous (it ends in a device-to-host copy), so a host clock around the bare library call (buffers made once) is
the call's time; warm-up calls first, then the median of the repetitions (and the 10th / 90th percentile as the
spread).  One JSON line per workload.

    python tools/time_new_points.py [--reps 50] [--warmup 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vieo_slam_amd import _lib, tri_search  # noqa: E402

BF = 47.9


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=round(float(np.median(ts)), 4), p10_ms=round(float(np.percentile(ts, 10)), 4),
                p90_ms=round(float(np.percentile(ts, 90)), 4))


def workload(name, warmup, reps, **kw):
    kf1, kf2s, _ = tri_search.make_tri_scene(21, **kw)
    if kw.get("rig"):  # rig frames: uright = -1 everywhere, the points come from the triangulation
        for k in [kf1] + kf2s:
            k.uright[:] = -1
        mk = lambda k: tri_search.TriStereo(k, BF, depth=np.full(len(k.keys), -1, np.float32))
    else:
        mk = lambda k: tri_search.TriStereo(k, BF)
    st1, st2s = mk(kf1), [mk(k) for k in kf2s]
    found = tri_search.SearchForTriangulation(kf1, kf2s)
    rows = [f[0] for f in found]
    out = tri_search.TriangulateNewPoints(kf1, st1, kf2s, st2s, rows)
    res = dict(workload=name, neighbours=len(kf2s), keys_kf1=len(kf1.keys), rows=int(sum(len(r) for r in rows)),
               new_points=int(sum(o[3] for o in out)), reps=reps, warmup=warmup)
    # the buffers are made once: the timed region is the library call alone
    L = _lib.lib()
    cap, stride, pairs, n_pairs, n_matches, status, x3d, x3d_f, n_new = tri_search.new_points_buffers(kf1, kf2s)
    recs = np.concatenate([k.rec for k in kf2s])
    srecs = np.concatenate([s.rec for s in st2s])
    a1, s1, a2, s2, n = kf1.rec.ctypes.data, st1.rec.ctypes.data, recs.ctypes.data, srecs.ctypes.data, len(kf2s)
    outs = (status.ctypes.data, x3d.ctypes.data, x3d_f.ctypes.data, n_new.ctypes.data)

    def search():
        assert L.vieo_search_for_triangulation(a1, a2, n, 0, 1, cap, stride, pairs.ctypes.data, n_pairs.ctypes.data,
                                               n_matches.ctypes.data) == 0

    def triangulate():  # on the rows the search left in `pairs`
        assert L.vieo_triangulate_new_points(a1, s1, a2, s2, n, 0.0, cap, stride, pairs.ctypes.data, n_pairs.ctypes.data,
                                             *outs) == 0

    def create():
        assert L.vieo_create_new_map_points(a1, s1, a2, s2, n, 0, 1, 0.0, cap, stride, pairs.ctypes.data,
                                            n_pairs.ctypes.data, n_matches.ctypes.data, *outs) == 0

    res["search"] = timed(search, warmup, reps)
    res["triangulate"] = timed(triangulate, warmup, reps)
    res["create"] = timed(create, warmup, reps)
    assert int(n_new.sum()) == res["new_points"]
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not _lib.lib().vieo_device_available():
        raise SystemExit("no gfx950 device: " + _lib.lib().vieo_last_error().decode())
    workload("undistorted_10x3000", a.warmup, a.reps, n_points=3000, n_neighbours=10)
    workload("kb8_rig_8", a.warmup, a.reps, rig="kb8", n_points=1500, n_neighbours=8)


if __name__ == "__main__":
    main()
