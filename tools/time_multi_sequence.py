"""Several live sequences on one GPU: vieo_track_frames (one call per lock step) against vieo_track_frame (one tracker per
sequence, called one after another in one thread).  Markdown table on stdout, one JSON line at the end.

  python tools/time_multi_sequence.py [--n 1,8,32,128,256] [--warmup 4] [--steps 12] [--seeds 16] [--baseline-max 32]

Per N: N sequences of the rectified stereo-inertial replay (tracker_multi.MultiTrackerReplay; `seeds` distinct rendered
sequences, sequence j uses seed j mod `seeds`: every sequence keeps its own map, key frames and local BAs), `warmup`
calls, then `steps` timed calls.  Reported per call: the call's wall time (vieo_track_output.ms_host) and GPU time
(ms_gpu, upload to download), median and mean; frames/s = N / median ms_host.  Two image paths: `planes` -- every frame is
decoded (copied) into its slot's pinned planes before the call, which then makes no host copy -- and `buffers` -- the
call copies the caller's images into the planes itself.  Calls that took the wider window are counted.
The baseline: the same frames through one vieo_tracker per sequence (tracker.TrackerReplay, images decoded into the
tracker's planes); its calls run one after another and each returns synchronised, so its frames/s is 1000 / median
ms_host whatever N is -- it runs min(N, baseline-max) trackers.  Every call of a step is timed, local BAs are not."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(ms):
    a = np.asarray(ms, np.float64)
    return float(np.median(a)), float(a.mean())


def time_multi(seqs, n, warmup, steps, into_planes):
    from vieo_slam_amd import replay
    from vieo_slam_amd.tracker_multi import MultiTrackerReplay
    M = MultiTrackerReplay(replay.HipStages(), n, into_planes=into_planes)
    for s in range(n):
        M.start(s, seqs[s % len(seqs)], warmup + steps + 1)
    widened_frames = []
    for c in range(warmup + steps):
        res = M.step()
        if c >= warmup:
            widened_frames.append(sum(int(o["widened"]) for o, _ in res))
    ms = M.stats["ms_call"][warmup:]
    M.close()
    host, gpu = _stats([m[0] for m in ms]), _stats([m[1] for m in ms])
    return dict(ms_host_median=host[0], ms_host_mean=host[1], ms_gpu_median=gpu[0], ms_gpu_mean=gpu[1],
                fps=1000.0 * n / host[0], widened_calls=sum(w > 0 for w in widened_frames),
                widened_frames=int(sum(widened_frames)))


def time_single(seqs, n, warmup, steps):
    from vieo_slam_amd import replay
    from vieo_slam_amd.tracker import TrackerReplay
    S = replay.HipStages()
    reps = []
    for j in range(n):
        r = TrackerReplay(seqs[j % len(seqs)], S)
        r.initialise()
        reps.append(r)
    for k in range(1, warmup + steps + 1):
        for r in reps:  # (frame-major: tracker after tracker, one thread)
            r.before_frame(k)
            args, ctx = r.track_args(k)
            pl = r.trk.planes
            pl[0][:], pl[1][:] = args["left"], args["right"]
            args["left"], args["right"] = pl[0], pl[1]
            o, v = r.trk.track(**args)
            r.apply_output(k, o, v, ctx, 0.0)
    ms = [m for r in reps for m in r.stats["ms_chain"][warmup:]]
    widened = sum(r.stats["widened"] for r in reps)
    for r in reps:
        r.close()
    host, gpu = _stats([m[0] for m in ms]), _stats([m[1] for m in ms])
    return dict(ms_host_median=host[0], ms_gpu_median=gpu[0], fps=1000.0 / host[0], trackers=n, widened_frames=widened)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1,8,32,128,256")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--seeds", type=int, default=16)
    ap.add_argument("--baseline-max", type=int, default=32)
    ap.add_argument("--paths", default="planes,buffers")
    a = ap.parse_args()
    from vieo_slam_amd.tracker_multi import make_sequences
    ns = [int(x) for x in a.n.split(",")]
    seqs = make_sequences(range(1, 1 + a.seeds), a.warmup + a.steps + 1, workers=16)
    base = time_single(seqs, min(max(ns), a.baseline_max), a.warmup, a.steps)
    rows = []
    print("| N | images | call ms (median / mean) | GPU ms (median / mean) | frames/s | x one tracker | calls widened |")
    print("|---|---|---|---|---|---|---|")
    for n in ns:
        for path in a.paths.split(","):
            r = time_multi(seqs, n, a.warmup, a.steps, path == "planes")
            r.update(n=n, images=path, ratio=r["fps"] / base["fps"])
            rows.append(r)
            print("| %d | %s | %.3f / %.3f | %.3f / %.3f | %.0f | %.2f | %d of %d |" % (
                n, path, r["ms_host_median"], r["ms_host_mean"], r["ms_gpu_median"], r["ms_gpu_mean"], r["fps"], r["ratio"],
                r["widened_calls"], a.steps), flush=True)
    print("\none tracker per sequence (%d trackers, calls one after another): call %.3f ms (GPU %.3f), %.0f frames/s, "
          "%d frames widened" % (base["trackers"], base["ms_host_median"], base["ms_gpu_median"], base["fps"], base["widened_frames"]))
    print(json.dumps(dict(metric="multi_sequence_tracking", warmup=a.warmup, steps=a.steps, seeds=a.seeds, baseline=base,
                          rows=rows)))


if __name__ == "__main__":
    main()
