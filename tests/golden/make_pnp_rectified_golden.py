"""Writes tests/golden/pnp_rectified_rows.npz: SHA-256 of the pass-A rows and pass-B records that vieo_pnp_create
returns for the rectified PnP scenes of tests/test_relocalization.py (seeds 100 ... 131, 40 sample rows, one batch).

Run on an MI355X from the repo root, with the library of the commit whose results are to be pinned (the parent of the
rig PnP instances; VIEO_LIB_PATH selects a build):
    python tests/golden/make_pnp_rectified_golden.py [OUT_DIR]
Two calls must give the same bytes, or nothing is written.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SEEDS = list(range(100, 132))
ROWS = 40


def scenes():
    from vieo_slam_amd import relocalization as rl
    out = []
    for seed in SEEDS:
        s = rl.make_pnp_scene(seed)
        out.append((s, rl.draw_samples(np.random.default_rng([seed, 1]), len(s["Xw"]), ROWS)))
    return out


def digests():
    """(rows, records): uint8 (32 seeds, 32) each -- SHA-256 over samples, Rt, count, mask of every row; over rec_row,
    Rt, count, mask of every record"""
    from vieo_slam_amd import relocalization as rl
    sc = scenes()
    solver = rl.PnPSolver([s for s, _ in sc], [smp for _, smp in sc], params=rl.RELOC_PNP_PARAMS)
    rows, recs = [], []
    for c in range(len(sc)):
        for tap, out in ((solver.rows(c), rows), (solver.records(c), recs)):
            h = hashlib.sha256()
            for a in tap:
                h.update(np.ascontiguousarray(a).tobytes())
            out.append(np.frombuffer(h.digest(), np.uint8))
    solver.close()
    return np.stack(rows), np.stack(recs)


if __name__ == "__main__":
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden")
    os.makedirs(out_dir, exist_ok=True)
    a, b = digests(), digests()
    if not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])):
        raise SystemExit("two calls differ: nothing written")
    np.savez_compressed(os.path.join(out_dir, "pnp_rectified_rows.npz"), seeds=np.array(SEEDS, np.int32),
                        n_rows=np.int32(ROWS), rows_sha256=a[0], records_sha256=a[1])
    print("pnp_rectified_rows.npz:", bytes(a[0][0]).hex()[:16], bytes(a[1][0]).hex()[:16], flush=True)
