"""Writes tests/golden/pose_batch_narrow_parent.npz: the results of the one-wavefront-per-frame PoseOptimization kernel
on the batch of pose_batch_narrow_cases.py, one record per distinct problem, bytes and all.

Run on an MI355X from the repo root, with the library of the commit whose results are to be pinned (the parent of the
two-wavefronts-per-SIMD kernel; VIEO_LIB_PATH selects a build):
    python tests/golden/make_pose_batch_narrow_golden.py [OUT_DIR]
Every repeat of a problem in the batch must give the bytes of its first occurrence, or nothing is written.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.golden import pose_batch_narrow_cases as cases  # noqa: E402


def pack(frames, res, outl):
    first = {}
    for i in range(cases.B):
        b, n = int(frames[i]["base"]["obs_begin"]), int(frames[i]["base"]["n_obs"])
        f = cases.fields_of(res[i], outl[b:b + n])
        k = cases.which(i)
        if k not in first:
            first[k] = f
        elif first[k] != f:
            raise SystemExit("problem %s differs at batch position %d: %s" % (
                cases.NAMES[k], i, [name for name in f if f[name] != first[k][name]]))
    out = {}
    for name in cases.FIELDS:
        out[name] = np.stack([np.frombuffer(first[k][name], np.uint8) for k in range(len(cases.NAMES))])
    out["outlier"] = np.concatenate([np.frombuffer(first[k]["outlier"], np.uint8) for k in range(len(cases.NAMES))])
    out["outlier_len"] = np.array([len(first[k]["outlier"]) for k in range(len(cases.NAMES))], np.int64)
    return out


if __name__ == "__main__":
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden")
    os.makedirs(out_dir, exist_ok=True)
    P, frames, obs = cases.build()
    res, outl = cases.run_hip(frames, obs)
    g = pack(frames, res, outl)
    np.savez_compressed(os.path.join(out_dir, "pose_batch_narrow_parent.npz"), **g)
    for k, name in enumerate(cases.NAMES):
        r = res[[i for i in range(cases.B) if cases.which(i) == k][0]]
        print(name, "status", int(r["base"]["status"]), "inliers", int(r["base"]["n_inliers"]), "iterations",
              int(r["base"]["lm_iterations"]), "trials", int(r["base"]["reserved"]), flush=True)
