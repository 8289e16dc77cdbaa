"""Times vieo_optimize_sim3 on the key frames of tools/time_loop_verify.py: V visits (1 / 4 / 16, one candidate each) of a
current key frame of --keys keys with --points map points in one call, against the same visits issued one by one through
single-visit calls, in one run, the two forms alternating.  The visits are what SearchBySim3 hands over: its match12
and a Sim3 a little off the true one.  A call packs its correspondences, uploads them once, launches k_sim3_optimize once
and ends in the copy back, so the host clock around it is device-synchronised.  Median of --repeat rounds after a warm-up
round, min ... max in brackets.  Reports, not thresholds: one call against many calls compares the code with itself.
Usage: python tools/time_loop_optimize.py [--keys 1200] [--points 300] [--repeat 30]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vieo_slam_amd import _lib  # noqa: E402
from vieo_slam_amd import loop_closing as lc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1200)
    ap.add_argument("--points", type=int, default=300)
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--visits", type=int, nargs="*", default=[1, 4, 16])
    a = ap.parse_args()
    if not _lib.lib().vieo_device_available():
        raise SystemExit("no gfx950 device: nothing to time")
    print("rounds per figure: %d (median, min ... max); key frames of %d keys, %d map points" % (a.repeat, a.keys, a.points))
    print("visits  one call [ms]                 one by one [ms]               correspondences / nInliers / trials per visit")
    for V in a.visits:
        s = lc.make_loop_pair_scene(400 + V, n_keys=a.keys, n_points=a.points, n_cands=V)
        empty = np.full(len(s["kf1"].keys), -1, np.int32)
        found = lc.SearchBySim3(s["kf1"], s["kf2s"], [(c,) + tuple(s["sim3"][c]) + (empty,) for c in range(V)])
        visits = []
        for c in range(V):
            s12, R12, t12 = (np.asarray(x, np.float64) for x in s["sim3"][c])
            visits.append((c, float(s12) * 1.01, lc.rodrigues(np.array([0.004, -0.005, 0.003])) @ R12, t12 + 0.03, found[c][0]))

        def batch():
            return lc.optimize_sim3_call(s["kf1"], s["kf2s"], visits)[1]

        def singly():
            return [lc.optimize_sim3_call(s["kf1"], [s["kf2s"][v[0]]], [(0,) + v[1:]])[1][0] for v in visits]

        a_out, b_out = batch(), singly()
        assert all(x["match12"].tobytes() == y["match12"].tobytes() and x["R12"].tobytes() == y["R12"].tobytes() for x, y in zip(a_out, b_out))
        ts = {batch: [], singly: []}
        for _ in range(a.repeat):
            for fn in (batch, singly):
                t0 = time.perf_counter()
                fn()
                ts[fn].append((time.perf_counter() - t0) * 1e3)
        fmt = lambda t: "%8.3f (%.3f ... %.3f)" % (np.median(t), np.min(t), np.max(t))
        print("%6d  %-28s  %-28s  %s" % (V, fmt(ts[batch]), fmt(ts[singly]),
                                         [(x["n_correspondences"], x["n_inliers"], sum(x["trials"])) for x in a_out][:4]))


if __name__ == "__main__":
    main()
