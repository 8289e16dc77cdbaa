"""Timing of the full BA's tile-sparse LDL^T (solver class 3) -- one JSON line.

  python tools/time_gba_sparse.py [--reps 3]

Cases, each in a child process (VIEO_LBA_SPARSE_SOLVE / VIEO_LBA_BIG_SOLVE are read once per process):
  vio400_sparse / vio400_dense  the 400-key-frame scale problem of tests/test_global_ba_scale.py (6001 unknowns), forced
                                tile-sparse / forced dense tiled solve, 2 iterations
  vio2000                       2 000 visual-inertial key frames with the scale vertex (30 001 unknowns), 5 iterations
  vision3000                    BundleAdjustment over 3 000 key frames (18 000 unknowns), 5 iterations
Per case: ms per call (the call returns after its stream synchronised; `reps` calls after a warm-up one, min / median /
max), ms per LM trial, vieo_lba_kernel_times per class of one more call with kernel timing on, stored tiles against
the dense lower triangle's, planned Schur tiles against the dense upper grid's, plan and arena bytes."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"vio400_sparse": "VIEO_LBA_SPARSE_SOLVE", "vio400_dense": "VIEO_LBA_BIG_SOLVE", "vio2000": None, "vision3000": None}


def _problem(case):
    from vieo_slam_amd import synth_ba
    from vieo_slam_amd.optimizer import Optimizer
    if case.startswith("vio"):
        n, pts_n, iters = (400, 4000, 2) if case.startswith("vio400") else (2000, 10000, 5)
        params, kfs, pts, close, obs, imu, gt = synth_ba.make_lba_vio_problem(7 if n == 400 else 31, n_local=n, n_fixed=1,
                                                                              n_points=pts_n, anchors=n // 2, span=5)
        pts = (pts / np.float32(1.02)).astype(np.float32)
        return lambda: Optimizer.GlobalBundleAdjustmentNavStatePRV(params, kfs, pts, obs, imu, iters, True, bScaleOpt=True)[2], n
    P, kfs, pts, obs, gt = synth_ba.make_lba_problem(33, n_local=3000, n_fixed=1, n_points=15000, anchors=1500, span=5)
    return lambda: Optimizer.BundleAdjustment(P, kfs, pts, obs, 5, True)[2], 3000


def child(case, reps):
    from vieo_slam_amd._lib import lib
    from vieo_slam_amd.optimizer import Optimizer
    call, n_kf = _problem(case)
    res = call()  # warm-up: arena allocation, code objects
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = call()
        ms.append((time.perf_counter() - t0) * 1e3)
    Optimizer.enable_kernel_timing(True)
    call()
    kt, _ = Optimizer.kernel_times()
    Optimizer.enable_kernel_timing(False)
    st = np.zeros(6, np.int64)
    lib().vieo_lba_sparse_stats(st.ctypes.data)
    trials = int(res["lm_trials"])
    out = dict(case=case, key_frames=n_kf, status=int(res["status"]), lm_trials=trials,
               ms_per_call=dict(min=min(ms), median=float(np.median(ms)), max=max(ms)),
               ms_per_trial=dict(min=min(ms) / trials, median=float(np.median(ms)) / trials, max=max(ms) / trials),
               kernel_ms={k: round(v["ms"], 3) for k, v in kt.items() if v["launches"]},
               kernel_launches={k: v["launches"] for k, v in kt.items() if v["launches"]})
    if "dense" not in case:
        out.update(stored_tiles=int(st[0]), dense_tiles=int(st[1]), schur_tiles=int(st[2]), schur_dense_tiles=int(st[3]),
                   plan_bytes=int(st[4]), arena_bytes=int(st[5]))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps)
        return
    line = {"tool": "time_gba_sparse", "reps": a.reps}
    for case, var in CASES.items():
        env = {k: v for k, v in os.environ.items() if k not in ("VIEO_LBA_SPARSE_SOLVE", "VIEO_LBA_BIG_SOLVE")}
        if var:
            env[var] = "1"
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, "--reps", str(a.reps)], env=env,
                           capture_output=True, text=True, timeout=1200)
        if p.returncode != 0:
            line[case] = {"error": p.returncode, "stderr": p.stderr[-2000:]}
            break
        line[case] = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(line))


if __name__ == "__main__":
    main()
