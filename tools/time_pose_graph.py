"""Times vieo_optimize_essential_graph (Optimizer::OptimizeEssentialGraph on the device) on synthetic trajectories with
one loop: 200 / 1000 / 2000 key frames on a circle with odometry drift, spanning-tree edges, covisibility edges to k - 2
and k - 3, the loop edge from the last key frame to the first, five map points per key frame.  Reports ms per call, ms
per LM trial and the kernel launches of a trial (3 per tile column of the factorisation + 6).

    python tools/time_pose_graph.py [--sizes 200 1000 2000] [--repeats 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vieo_slam_amd import pose_graph as pg  # noqa: E402


def make_case(n_kf, seed=1):
    tr = pg.make_loop_trajectory(seed, n_kf=n_kf, drift_rot=0.01 / np.sqrt(n_kf / 24), drift_trans=0.03 / np.sqrt(n_kf / 24),
                                 radius=5.0 * n_kf / 24)
    cov = []
    for k in range(n_kf):
        cov += [(k, k - b, w) for b, w in ((1, 200), (2, 150), (3, 120)) if k - b >= 0]
    ei, ej, kind, info = pg.essential_graph_edges(np.ones(n_kf), tr["parent"], [], cov, {tr["cur_kf"]: [tr["loop_kf"]]},
                                                  tr["cur_kf"], tr["loop_kf"])
    rng = np.random.default_rng(seed)
    Pw = (rng.standard_normal((5 * n_kf, 3)) * 5).astype(np.float32)
    ref = np.repeat(np.arange(n_kf, dtype=np.int32), 5)
    return dict(Scw=tr["Scw"], Scw_prior=tr["Scw_prior"], valid=np.ones(n_kf, np.uint8), fixed_kf=0, edge_i=ei, edge_j=ej,
                edge_kind=kind, edge_info=info, Pw=Pw, ref_kf=ref, fix_scale=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[200, 1000, 2000])
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    rows = []
    for n_kf in a.sizes:
        c = make_case(n_kf)
        out = pg.optimize_essential_graph(**c)  # warm-up: allocations, code objects
        times = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            out = pg.optimize_essential_graph(**c)
            times.append((time.perf_counter() - t0) * 1e3)
        ms = float(np.median(times))
        tiles = (out["n_unknowns"] + 63) // 64
        rows.append(dict(key_frames=n_kf, edges=len(c["edge_i"]), unknowns=out["n_unknowns"], tile_columns=tiles,
                         iterations=out["lm_iterations"], trials=out["lm_trials"], chi2_initial=out["chi2_initial"],
                         chi2_final=out["chi2_final"], ms_per_call=round(ms, 2), ms_per_trial=round(ms / max(out["lm_trials"], 1), 2),
                         launches_per_trial=3 * tiles + 6))
        print(json.dumps(rows[-1]))
    print("| key frames | edges | unknowns | iterations / trials | ms per call | ms per trial | launches per trial |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %d | %d | %d | %d / %d | %.1f | %.2f | %d |" % (r["key_frames"], r["edges"], r["unknowns"], r["iterations"],
                                                             r["trials"], r["ms_per_call"], r["ms_per_trial"], r["launches_per_trial"]))


if __name__ == "__main__":
    main()
