"""Times vieo_imu_init (IMUInitialization::TryInitVIO for a batch of sequences): 1 sequence of --kf key frames, then 32 and
256 of them in one call.  The arrays are packed once; a call uploads them once, runs its chain of launches and ends in the
copy back, so the host clock around it is device-synchronised.  Median of --repeat calls after a warm-up call, min ... max
in brackets.  Reports, not thresholds.
--trace DIR: after the timing, ONE `rocprofv3 --kernel-trace` run of its own (a fresh child process: this script with
--child) per batch size, and the time per launch of the chain from its rocpd result, warm-up call excluded.
Usage: python tools/time_imu_init.py [--kf 60] [--repeat 3] [--sequences 1 32 256] [--trace DIR]"""
import argparse
import glob
import os
import sqlite3
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vieo_slam_amd import _lib  # noqa: E402
from vieo_slam_amd import imu_init as ii  # noqa: E402


def packed(n_seq, n_kf):
    protos = [ii.make_init_case(3 + k, n_kf, step=5, n_points=2000) for k in range(min(n_seq, 8))]
    return ii.pack([protos[b % len(protos)] for b in range(n_seq)])


def per_launch(db_path, calls):
    """kernel name -> (launches per call, mean us per call) over the last `calls` calls of the trace"""
    db = sqlite3.connect(db_path)
    cols = [r[1] for r in db.execute("pragma table_info(kernels)")]
    name_col = "name" if "name" in cols else [c for c in cols if "name" in c][0]
    rows = db.execute("select %s, start, end from kernels order by start" % name_col).fetchall()
    per_call = len(rows) // (calls + 1)  # the warm-up call first
    rows = rows[per_call:]
    out = []
    for i in range(per_call):  # the chain's launches in order
        d = [rows[c * per_call + i][2] - rows[c * per_call + i][1] for c in range(calls)]
        out.append((rows[i][0].replace("(anonymous namespace)::", "").split("(")[0], float(np.mean(d)) / 1e3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kf", type=int, default=60)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--sequences", type=int, nargs="*", default=[1, 32, 256])
    ap.add_argument("--trace", default=None)
    ap.add_argument("--child", type=int, default=0)
    a = ap.parse_args()
    if not _lib.lib().vieo_device_available():
        raise SystemExit("no gfx950 device: nothing to time")
    if a.child:  # the traced run: a warm-up call and --repeat calls, nothing else
        pk = packed(a.child, a.kf)
        for _ in range(a.repeat + 1):
            _lib.check(ii.call(pk), "vieo_imu_init")
        return
    print("%d key frames per sequence, 2000 points each; median of %d calls after a warm-up (min ... max)" % (a.kf, a.repeat))
    print("sequences  call [ms]                        per sequence [us]  statuses  sweeps")
    for n_seq in a.sequences:
        pk = packed(n_seq, a.kf)
        _lib.check(ii.call(pk), "vieo_imu_init")
        ts = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            _lib.check(ii.call(pk), "vieo_imu_init")
            ts.append((time.perf_counter() - t0) * 1e3)
        r = pk["res"]
        print("%9d  %8.3f (%.3f ... %.3f)  %12.1f  %s  %s" % (n_seq, np.median(ts), min(ts), max(ts), np.median(ts) * 1e3 / n_seq,
                                                             sorted(set(r["status"].tolist())), r["sweeps"][0].tolist()))
    if not a.trace:
        return
    for n_seq in a.sequences:
        d = os.path.join(a.trace, "seq%d" % n_seq)
        os.makedirs(d, exist_ok=True)
        subprocess.check_call(["rocprofv3", "--kernel-trace", "-d", d, "-o", "out", "--", sys.executable, os.path.abspath(__file__),
                               "--child", str(n_seq), "--kf", str(a.kf), "--repeat", str(a.repeat)],
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
        if not dbs:
            print("%d sequences: no rocpd result under %s" % (n_seq, d))
            continue
        chain = per_launch(dbs[0], a.repeat)
        merged = []  # consecutive launches of one kernel (the slices of a pre-integration pass) as one entry
        for k, t in chain:
            k = k.split("::")[-1]
            if merged and merged[-1][0] == k:
                merged[-1] = (k, merged[-1][1] + t, merged[-1][2] + 1)
            else:
                merged.append((k, t, 1))
        print("%d sequences, per launch [us] (sum %.1f): %s" % (n_seq, sum(t for _, t in chain), ", ".join(
            "%s%s %.1f" % (k, " x %d" % c if c > 1 else "", t) for k, t, c in merged)))


if __name__ == "__main__":
    main()
