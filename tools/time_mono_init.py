"""Times the matcher of the monocular initialisation, vieo_search_for_initialization (ORBmatcher::SearchForInitialization),
on synthetic frame pairs of --keys keys (initialization.make_search_pair, window 100 as Tracking::MonocularInitialization
calls it; 32 scenes, repeated for the 256): one pair, 32 pairs and 256 pairs in ONE call each, and 32 one-pair calls for
the same 32 pairs, alternating with the batched calls so that all see the same machine.  The 32-pair call and the single
calls must give the same matches, or the tool fails.  Each call is synchronous (it ends in the copy back and the host
walk), so a host clock around it measures the whole call.  Per figure: a warm-up call, then --repeat calls; median
(min ... max) in milliseconds.  Reports, not thresholds.
Usage: python tools/time_mono_init.py [--repeat 30] [--keys 1000]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vieo_slam_amd import _lib  # noqa: E402
from vieo_slam_amd import initialization as ini  # noqa: E402


def stats(ts):
    return "%9.3f (%.3f ... %.3f)" % (float(np.median(ts)), float(np.min(ts)), float(np.max(ts)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--keys", type=int, default=1000)
    a = ap.parse_args()
    if not _lib.lib().vieo_device_available():
        raise SystemExit("no gfx950 device: " + _lib.lib().vieo_last_error().decode())
    pairs, bounds = [], None
    for s in range(32):
        F1, F2, prev, bounds = ini.make_search_pair(1000 + s, a.keys, a.keys)
        pairs.append((F1, F2, prev, ini.WINDOW_INIT))
    pairs = pairs * 8  # (256 pairs: the 32 scenes eight times over; the call treats every pair on its own)

    def call(lo, hi):
        return ini.SearchForInitialization(pairs[lo:hi], bounds)

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    batched = call(0, 32)
    single = [call(p, p + 1)[0] for p in range(32)]
    for b, s in zip(batched, single):
        if not (np.array_equal(b[0], s[0]) and b[1] == s[1] and np.array_equal(b[2], s[2])):
            raise SystemExit("the 32-pair call and the one-pair calls differ")
    call(0, 256), call(0, 1)
    t1, t32, t32x1, t256 = [], [], [], []
    for _ in range(a.repeat):
        t1.append(clock(lambda: call(0, 1)))
        t32.append(clock(lambda: call(0, 32)))
        t32x1.append(clock(lambda: [call(p, p + 1) for p in range(32)]))
        t256.append(clock(lambda: call(0, 256)))
    n = [r[1] for r in batched]
    listed = sum(len(lst) for lst in ini.search_for_initialization_tap(a.keys, 0))
    print("vieo_search_for_initialization, %d-key frames, window %d, %d repeats, ms: median (min ... max)" % (a.keys, ini.WINDOW_INIT, a.repeat))
    print("  matches per pair: %d ... %d; listed candidates of pair 0 of the last call: %d" % (min(n), max(n), listed))
    print("  1 pair, one call          %s" % stats(t1))
    print("  32 pairs, one call        %s" % stats(t32))
    print("  32 pairs, 32 calls        %s" % stats(t32x1))
    print("  256 pairs, one call       %s" % stats(t256))
    print("  one 32-pair call / 32 one-pair calls: %.3f" % (float(np.median(t32)) / float(np.median(t32x1))))
    print("  per pair in the 256-pair call: %.4f ms" % (float(np.median(t256)) / 256))


if __name__ == "__main__":
    main()
