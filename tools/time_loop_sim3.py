"""Times the first half of loop verification:
  - vieo_sim3_create (all hypotheses of all candidates in one launch, the tables copied back: the call ends in a device
    synchronisation) for 1 / 4 / 16 candidates of 60 and 300 correspondences at 300 sample rows, with one iterate(5) per
    candidate, which is a look-up;
  - vieo_search_by_bow_kf of a key frame of 1200 keys against 1 / 4 / 16 candidates of 1200 keys.
Median of --repeat calls after a warm-up call, on a host clock.  Reports, not thresholds.
Usage: python tools/time_loop_sim3.py [--rows 300] [--repeat 50]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vieo_slam_amd import _lib  # noqa: E402
from vieo_slam_amd import loop_closing as lc  # noqa: E402


def median_ms(fn, repeat):
    fn()
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=300)
    ap.add_argument("--repeat", type=int, default=50)
    a = ap.parse_args()
    if not _lib.lib().vieo_device_available():
        raise SystemExit("no gfx950 device: nothing to time")
    print("runs per figure: %d (median, min ... max)" % a.repeat)
    print("candidates  correspondences  rows  vieo_sim3_create + iterate(5) [ms]")
    for n in (60, 300):
        for K in (1, 4, 16):
            scenes = [lc.make_sim3_scene(200 + c, n) for c in range(K)]
            samples = [lc.draw_samples(np.random.default_rng([200 + c, 1]), n, a.rows) for c in range(K)]

            def device():
                solver = lc.Sim3Solver(scenes, samples, params=lc.LOOP_SIM3_PARAMS)
                found = [solver.iterate(c, 5).found for c in range(K)]
                solver.close()
                return found

            print("%10d  %15d  %4d  %10.3f (%.3f ... %.3f)" % ((K, n, a.rows) + median_ms(device, a.repeat)))
    print("candidates  keys  vieo_search_by_bow_kf [ms]")
    for K in (1, 4, 16):
        kf1, cands = lc.make_bow_kf_scene(300 + K, n_cands=K + 1, n_keys=1200, n_nodes=120)
        cands = cands[:K]  # (the last one of the scene shares no node)
        print("%10d  %4d  %10.3f (%.3f ... %.3f)" % ((K, 1200) + median_ms(lambda: lc.SearchByBoWKF(kf1, cands, 0.75, True), a.repeat)))


if __name__ == "__main__":
    main()
