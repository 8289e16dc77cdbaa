"""One JSON line that pins down a Python replay run: hashes of the trajectory, of the map arrays and of every key frame's
state, the observation table in a canonical form (a key index and a one-key tuple are written the same), the stats without
the timings, and how often the erase path and the several-keys-per-key-frame path were taken.  Two commits computed the same
thing iff their lines are equal.  Only names that every commit with these replays has are used, so the file runs unchanged
against an older tree on PYTHONPATH:
    python tools/replay_digest.py --mode rig --rig kb8 --cams 4 --features 1500 --seed 5 --frames 32 --lag 3
    PYTHONPATH=/path/to/older/tree python tools/replay_digest.py ...      (the package and tests/ come from there)
--stages oracle needs no GPU (modes vio, vision, rig); chained and the *tracker modes are one-call paths of the library."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

if not os.environ.get("PYTHONPATH"):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vieo_slam_amd import replay, replay_modes as rm, tracker  # noqa: E402


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def make(a):
    kw = dict(lba_lag=a.lag)
    pf = dict(prefetch=bool(a.prefetch))
    rig = a.mode.startswith("rig")
    seq = rm.RigSequence(a.seed, a.frames, a.rig, a.cams) if rig else replay.Sequence(a.seed, a.frames)
    if a.stages == "oracle":
        from tests import oracle_lib, replay_oracle as ro
        assert a.mode in ("vio", "vision", "rig"), "the one-call modes run on the library only"
        orc = oracle_lib.load()
        S = (ro.OracleRigStages(orc, a.features, a.cams) if rig else ro.OracleVisionStages(orc) if a.mode == "vision"
             else ro.OracleStages(orc))
    else:
        S = (rm.HipRigStages(a.features, a.cams) if rig else rm.HipVisionStages() if a.mode.startswith("vision")
             else replay.HipStages())
    if a.mode == "vio":
        return seq, replay.Replay(seq, S, **kw)
    if a.mode == "chained":
        return seq, replay.ChainedReplay(seq, S, **kw)
    if a.mode == "tracker":
        return seq, tracker.TrackerReplay(seq, S, **pf, **kw)
    if a.mode == "vision":
        return seq, rm.VisionReplay(seq, S, **kw)
    if a.mode == "vision_tracker":
        return seq, rm.VisionTrackerReplay(seq, S, **pf, **kw)
    if a.mode == "rig":
        return seq, rm.RigReplay(seq, S, a.features, **kw)
    return seq, rm.RigTrackerReplay(seq, S, a.features, **pf, **kw)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--mode", required=True, choices=["vio", "chained", "tracker", "vision", "vision_tracker", "rig", "rig_tracker"])
    p.add_argument("--stages", default="oracle", choices=["oracle", "hip"])
    p.add_argument("--seed", type=int, default=2)
    p.add_argument("--frames", type=int, default=62)
    p.add_argument("--lag", type=int, default=0)
    p.add_argument("--prefetch", type=int, default=0)
    p.add_argument("--rig", default="radtan")
    p.add_argument("--cams", type=int, default=2)
    p.add_argument("--features", type=int, default=1200)
    a = p.parse_args()
    seq, R = make(a)
    erased = [0]
    apply_ = R._lba_apply

    def counting(job):  # (rows flagged by a local BA whose write-back is taken)
        if int(job["res"]["status"]) == 0:
            erased[0] += int(np.count_nonzero(job["erase"]))
        return apply_(job)
    R._lba_apply = counting
    traj = R.run(a.frames)
    if hasattr(R, "close"):
        R.close()
    keys = lambda v: [int(i) for i in np.atleast_1d(v)]  # noqa: E731
    table = [[[int(kid), keys(v)] for kid, v in sorted(ob.items())] for ob in R.mp_obs]
    out = dict(mode=a.mode, stages=a.stages, lag=a.lag, prefetch=a.prefetch, frames=a.frames, seed=a.seed,
               traj=sha(traj), map={n: sha(getattr(R, n)) for n in ("mp_X", "mp_bad", "mp_normal", "mp_maxd", "mp_mind")},
               kf_nav=[sha(k.nav) for k in R.kfs], kf_mp_ref=[sha(k.mp_ref) for k in R.kfs],
               mp_obs=hashlib.sha256(json.dumps(table).encode()).hexdigest(), n_points=len(table),
               n_observations=sum(len(ks) for ob in table for _, ks in ob),
               stats={k: v for k, v in R.stats.items() if not k.startswith("ms_")}, erased=erased[0],
               lists_longer_than_one=sum(1 for ob in table for _, ks in ob if len(ks) > 1))
    print(json.dumps(out, sort_keys=True, default=str))


if __name__ == "__main__":
    main()
