"""One sha256 per RANSAC handle of fixed scenes, and one per chain that runs through such handles: two commits' libraries
computed the same bytes iff their lines are equal.  Handles: the rectified PnP, the PnP of a radtan2 rig frame, the Sim3
solver; each once with the library's own draw (seed 5) and once with a caller's table; 64 rows, candidates of 60
correspondences and one of 129 (three mask words).  A hash covers rows(), records() and usun() where the handle has them,
info() of every candidate, the results and info() after each of four iterate(c, 5) calls, and estimate() for Sim3.
Chains: Relocalization, RelocalizationRig and ComputeSim3 on one scene each (pose, matches, trace).  Only names every
commit with these handles has are used, so the file runs unchanged against another build:
    python tools/ransac_digest.py
    VIEO_LIB_PATH=/path/to/another/libvieo_hot.so python tools/ransac_digest.py"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vieo_slam_amd import loop_closing as lc  # noqa: E402
from vieo_slam_amd import relocalization as rl  # noqa: E402

SEEDS, ROWS, N, N_LONG = (100, 101, 102, 103), 64, 60, 129


class Digest:
    def __init__(self):
        self.h = hashlib.sha256()

    def add(self, *items):
        for a in items:
            if a is None:
                self.h.update(b"none")
            elif isinstance(a, dict):
                self.h.update(repr(sorted(a.items())).encode())
            elif isinstance(a, (tuple, list)):
                self.add(*a)
            else:
                a = np.ascontiguousarray(a)
                self.h.update(str((a.dtype.str, a.shape)).encode())
                self.h.update(a.tobytes())

    def hex(self):
        return self.h.hexdigest()


def handle_digest(solver, n_cands, kind):
    d = Digest()
    for c in range(n_cands):
        d.add(solver.rows(c), solver.info(c))
        if kind != "sim3":
            d.add(solver.records(c))
        if kind == "rig":
            d.add(solver.usun(c))
    for call in range(4):
        for c in range(n_cands):
            r = solver.iterate(c, 5)
            d.add(int(r.found), r.Tcw if kind != "sim3" else r.T12, r.inliers, int(r.n_inliers), int(r.no_more), int(r.row), solver.info(c))
            if kind == "sim3":
                d.add(solver.estimate(c))
    solver.close()
    return d.hex()


def tables(sizes, set_size, own):
    """None: the library's draw; else a caller's table per candidate"""
    if own:
        return None
    if set_size == 4:
        return [rl.draw_samples(np.random.default_rng([7, c]), n, ROWS) for c, n in enumerate(sizes)]
    return [lc.draw_samples(np.random.default_rng([7, c]), n, ROWS) for c, n in enumerate(sizes)]


def main():
    sizes = [N] * len(SEEDS) + [N_LONG]
    for own in (True, False):
        tag = "library's draw" if own else "caller's table"
        kw = dict(samples=tables(sizes, 4, own), n_rows=ROWS, seed=5, params=rl.RELOC_PNP_PARAMS)
        scenes = [rl.make_pnp_scene(s, n) for s, n in zip(SEEDS + (104,), sizes)]
        print("pnp rectified, %s: %s" % (tag, handle_digest(rl.PnPSolver(scenes, **kw), len(scenes), "pnp")))
        scenes = [rl.make_pnp_rig_scene(s, "radtan2", n, plane_z=1.0) for s, n in zip(SEEDS + (104,), sizes)]
        print("pnp radtan2 rig, %s: %s" % (tag, handle_digest(rl.PnPSolver(scenes, rig=scenes[0]["rig"]["pnp"], **kw), len(scenes), "rig")))
        scenes = [lc.make_sim3_scene(s, N, fix_scale=bool(s & 1)) for s in SEEDS] + [lc.make_sim3_scene(104, N, n_cams=2),
                                                                                     lc.make_sim3_scene(105, N_LONG)]
        kw = dict(samples=tables([N] * 5 + [N_LONG], 3, own), n_rows=ROWS, seed=5, params=lc.LOOP_SIM3_PARAMS)
        print("sim3, %s: %s" % (tag, handle_digest(lc.Sim3Solver(scenes, **kw), len(scenes), "sim3")))
    frame, cands, _ = rl.make_reloc_scene(1, "widen")
    o = rl.Relocalization(frame, cands, n_rows=ROWS, seed=5)
    d = Digest()
    d.add(int(o["found"]), o["cand"], o["n_good"], o["Tcw"], o["nav"], o["mp_ref"], o["outlier"], o["trace"])
    print("Relocalization (found %d): %s" % (o["found"], d.hex()))
    frame, rig, cands, _ = rl.make_reloc_rig_scene(1, "widen", "radtan2", plane_z=1.0)
    o = rl.RelocalizationRig(frame, rig, cands, n_rows=ROWS, seed=5)
    d = Digest()
    d.add(int(o["found"]), o["cand"], o["n_good"], o["Tcw"], o["nav"], o["mp_ref"], o["outlier"], o["trace"])
    print("RelocalizationRig (found %d): %s" % (o["found"], d.hex()))
    s = lc.make_compute_sim3_scene(31)
    ok, o = lc.ComputeSim3(s["kf1"], s["kf2s"], s["loop_points_of"], n_rows=ROWS, seed=5)
    d = Digest()
    d.add(int(ok), o["cand"], o["Scw"], np.float64(o["s"]), o["R"], o["t"], o["matched"], o["n_total_matches"], np.array(o["trace"], np.int64))
    print("ComputeSim3 (%d): %s" % (ok, d.hex()))


if __name__ == "__main__":
    main()
