"""Times the relocalisation pieces for K = 1, 4, 8 candidates of 150 matches each:
  - the device PnP: vieo_pnp_create (pass A over all K x S sample rows, the records, pass B) plus one iterate(5) per
    candidate, and the SearchByBoW batch over K key frames of 1000 keys;
  - the whole chain, vieo_relocalize, on the "widen" (3 candidates) and "direct" (1 candidate) scenes of the tests;
  - beside it the Python restatement of tests/reloc_ref.py on the host, which like the reference evaluates one
    hypothesis after the other and stops at the first success.
Every figure is a median (min ... max).  Reports, not thresholds.  Usage: python tools/time_relocalization.py [--rows 320] [--repeat 20]
--rig: the PnP of a rig frame (radtan2, kb8x4) beside the rectified one at the same sizes, and the rig chain."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import reloc_ref as ref  # noqa: E402
from vieo_slam_amd import relocalization as rl  # noqa: E402


def median_ms(fn, repeat):
    """median (min ... max) of `repeat` calls after a warm-up call, as text"""
    fn()
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return "%.3f (%.3f ... %.3f)" % (float(np.median(ts)), float(np.min(ts)), float(np.max(ts)))


def rig_table(a):
    """--rig: the device PnP (create + one iterate(5) per candidate) of a rig frame, kb8x4 and radtan2, beside the
    rectified one at the same sizes from the same run; the chain on the rig "widen" / "direct" scenes.  Median of
    a.repeat calls after a warm-up, with the smallest and the largest."""
    print("candidates  rows  rectified PnP [ms]  radtan2 PnP [ms]  kb8x4 PnP [ms]")
    for K in (1, 4, 8):
        samples = [rl.draw_samples(np.random.default_rng([200 + c, 1]), a.matches, a.rows) for c in range(K)]
        row, found = [], []
        for rig_kind in (None, "radtan2", "kb8x4"):
            if rig_kind is None:
                scenes, rig = [rl.make_pnp_scene(200 + c, a.matches) for c in range(K)], None
            else:  # (map points on the plane z = 1 of their camera: where the reference's usun is exact and a pose is found)
                scenes = [rl.make_pnp_rig_scene(200 + c, rig_kind, a.matches, plane_z=1.0) for c in range(K)]
                rig = scenes[0]["rig"]["pnp"]

            def device():
                solver = rl.PnPSolver(scenes, samples, params=rl.RELOC_PNP_PARAMS, rig=rig)
                found = [solver.iterate(c, 5).found for c in range(K)]
                solver.close()
                return found

            found.append(sum(device()))
            row.append(median_ms(device, a.repeat))
        print("%10d  %4d  %s  %s  %s   (poses found: %s)" % (K, a.rows, *row, found))
    print("scene   rig      device chain [ms]")
    for rig_kind in ("radtan2", "kb8x4"):
        for kind in ("widen", "direct"):
            frame, rig, cands, _ = rl.make_reloc_rig_scene(1, kind, rig_kind, plane_z=1.0)
            ok = rl.RelocalizationRig(frame, rig, cands, n_rows=a.rows, seed=1)["found"]
            print("%-6s  %-7s  %s   (found: %s)" % (kind, rig_kind, median_ms(
                lambda: rl.RelocalizationRig(frame, rig, cands, n_rows=a.rows, seed=1), a.repeat), ok))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=320)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--matches", type=int, default=150)
    ap.add_argument("--rig", action="store_true", help="the rig PnP and chain beside the rectified PnP")
    a = ap.parse_args()
    if a.rig:
        return rig_table(a)
    print("candidates  rows  device PnP [ms]  restated PnP on the host [ms]  device SearchByBoW [ms]")
    for K in (1, 4, 8):
        scenes = [rl.make_pnp_scene(200 + c, a.matches) for c in range(K)]
        samples = [rl.draw_samples(np.random.default_rng([200 + c, 1]), a.matches, a.rows) for c in range(K)]

        def device():
            solver = rl.PnPSolver(scenes, samples, params=rl.RELOC_PNP_PARAMS)
            found = [solver.iterate(c, 5).found for c in range(K)]
            solver.close()
            return found

        def host():
            return [ref.PnPSolverRef(s["Xw"], s["uv"], s["sigma2"], s["key_index"], s["n_frame_keys"], s["K"], smp,
                                     rl.RELOC_PNP_PARAMS).iterate(5).found for s, smp in zip(scenes, samples)]

        frame, kfs = rl.make_bow_scene(300 + K, n_kfs=K, n_keys=1000, n_nodes=120)
        assert all(device()) and all(host())
        print("%10d  %4d  %s  %s  %s" % (K, a.rows, median_ms(device, a.repeat), median_ms(host, max(a.repeat // 4, 2)),
                                         median_ms(lambda: rl.SearchByBoW(kfs, frame, 0.75, True), a.repeat)))
    from tests import oracle_lib
    orc = oracle_lib.load()
    print("scene   device chain [ms]  restated chain on the host [ms]")
    for kind in ("widen", "direct"):
        frame, cands, _ = rl.make_reloc_scene(1, kind)
        n = [int((ref.search_by_bow(c.bow, frame.bow, 0.75, True)[0] >= 0).sum()) for c in cands]
        samples = [rl.draw_samples(np.random.default_rng([1, i]), max(k, 4), a.rows) for i, k in enumerate(n)]
        assert rl.Relocalization(frame, cands, samples)["found"]
        print("%-6s  %s  %s" % (kind, median_ms(lambda: rl.Relocalization(frame, cands, samples), a.repeat),
                                median_ms(lambda: ref.relocalize(frame, cands, samples, ref.RefPnPBatch, orc, rl.RELOC_PNP_PARAMS), 2)))


if __name__ == "__main__":
    main()
