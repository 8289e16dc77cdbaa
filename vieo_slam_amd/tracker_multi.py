"""ctypes mirror of the multi-sequence tracker (include/vieo_hot.h: vieo_tracker_multi_*, vieo_track_frames) and a
replay that drives it: `MultiTrackerReplay` advances several `replay.Sequence`s in lock step, one frame of each per
call.  Each sequence keeps its own map, key frames and local BAs on the host, as in `tracker.TrackerReplay` (whose
input building and output handling it shares); only the frame tracking is batched."""
import ctypes
import time

import numpy as np

from ._lib import check, lib
from .ba_types import NAVSTATE_DTYPE
from .tracker import TRACK_INPUT_DTYPE, TRACK_OUTPUT_DTYPE, TRACKER_PARAMS_DTYPE, TrackerReplay, euroc_params, fill_track_input, \
    output_views


class MultiTracker:
    """vieo_tracker_multi: `track` takes one frame of each of several sequences (slot -> Tracker.track's keyword
    arguments) and returns, per frame, the output record and the numpy views of its arrays (valid until the next call)."""

    def __init__(self, params, max_sequences):
        L = lib()
        self.params = np.ascontiguousarray(params, TRACKER_PARAMS_DTYPE).reshape(1)
        self.max_sequences = int(max_sequences)
        h = ctypes.c_void_p()
        check(L.vieo_tracker_multi_create(ctypes.byref(h), self.params.ctypes.data, self.max_sequences),
              "vieo_tracker_multi_create")
        self.h = h
        w, hh = int(self.params[0]["width"]), int(self.params[0]["height"])
        self.planes, self._ptrs = [], []
        for s in range(self.max_sequences):
            pl, pt = [], []
            for c in range(2):
                a = ctypes.c_void_p()
                check(L.vieo_tracker_multi_image_buffer(h, s, c, ctypes.byref(a)), "vieo_tracker_multi_image_buffer")
                pl.append(np.ctypeslib.as_array((ctypes.c_uint8 * (w * hh)).from_address(a.value)).reshape(hh, w))
                pt.append(a.value)
            self.planes.append(pl)
            self._ptrs.append(pt)
        self.inp = np.zeros(self.max_sequences, TRACK_INPUT_DTYPE)
        self.out = np.zeros(self.max_sequences, TRACK_OUTPUT_DTYPE)
        self.last_rc = 0

    def close(self):
        if self.h:
            lib().vieo_tracker_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset_slot(self, slot):
        check(lib().vieo_tracker_multi_reset_slot(self.h, int(slot)), "vieo_tracker_multi_reset_slot")

    def call(self, slots, records):
        """vieo_track_frames on prepared vieo_track_input records: the return code (no exception)"""
        sl = np.ascontiguousarray(slots, np.int32)
        n = len(sl)
        rec = np.ascontiguousarray(records, TRACK_INPUT_DTYPE)
        self.last_rc = lib().vieo_track_frames(self.h, n, sl.ctypes.data, rec.ctypes.data, self.out.ctypes.data)
        return self.last_rc

    def record(self, slot, keep, left, right, imu, t_ref, t_cur, nav_ref, nav_last, prior, last_points, last_track_depth,
               local_points, local_desc, local_alias, local_version, next_images=None, use_prefetched=False, next_imu=None):
        """one frame's vieo_track_input record (the arrays it points at are appended to keep).  Images that are the slot's
        pinned planes go by pointer without a copy."""
        r = np.zeros(1, TRACK_INPUT_DTYPE)
        i = r[0]
        ptrs = []
        for c, img in enumerate((left, right)):
            if 0 <= slot < self.max_sequences and img is self.planes[slot][c]:
                ptrs.append(self._ptrs[slot][c])
            else:
                img = np.ascontiguousarray(img, np.uint8)
                keep.append(img)
                ptrs.append(img.ctypes.data)
        i["left"], i["right"] = ptrs
        assert next_images is None and not use_prefetched and next_imu is None, "no frame pipelining in vieo_track_frames"
        fill_track_input(i, self.params[0]["width"], imu, t_ref, t_cur, nav_ref, nav_last, prior, last_points, last_track_depth,
                         local_points, local_desc, local_alias, local_version, keep)
        return r

    def track(self, frames):
        """frames: list of (slot, Tracker.track keyword arguments) -> list of (output record, views)"""
        keep = []
        slots = [int(s) for s, _ in frames]
        rec = np.concatenate([self.record(s, keep, **a) for s, a in frames])
        check(self.call(slots, rec), "vieo_track_frames")
        res = []
        for j in range(len(frames)):
            o = self.out[j]
            res.append((o, output_views(o, int(rec[j]["n_local"]))))
        return res


class _LaneReplay(TrackerReplay):
    """one sequence of the lock-step replay: TrackerReplay without a tracker of its own"""

    def _make_tracker(self, max_local_points):
        return None


def _vision_lane():
    from .replay_modes import VisionTrackerReplay

    class _VisionLaneReplay(VisionTrackerReplay):
        def _make_tracker(self, max_local_points):
            return None
    return _VisionLaneReplay


class MultiTrackerReplay:
    """Several sequences tracked in lock step through one vieo_tracker_multi: `start` puts a sequence in a slot,
    `step` tracks the next frame of every running sequence in ONE call, `run` does both for a list of sequences.
    vision=True: the vision-only replay (replay_modes.VisionTrackerReplay) in every slot.  into_planes=True: every frame's
    images are copied ("decoded") into its slot's pinned planes before the call, which then makes no host copy.  Keyword
    arguments go to every sequence's replay (th_last, kf_every, ...)."""

    def __init__(self, stages, max_sequences, max_local_points=16384, vision=False, into_planes=False, **kw):
        self.S, self.kw, self.vision, self.into_planes = stages, kw, bool(vision), bool(into_planes)
        self.max_local_points = max_local_points
        self.max_sequences = int(max_sequences)
        self.mt = None
        self.lanes = {}      # slot -> [replay, next frame, frames to run]
        self.finished = []   # (slot, replay) in the order they ended
        self.stats = dict(calls=0, frames=0, widened_calls=0, ms_call=[])

    def _tracker(self, seq):
        if self.mt is None:
            th_last, th_local = self.kw.get("th_last", 7.0), self.kw.get("th_local", 1.0 if self.vision else 2.0)
            prm = euroc_params(self.max_local_points, th_last, th_local, seq.noise[0])
            if self.vision:
                from .replay_modes import NFEAT_VISION
                prm[0]["n_features"], prm[0]["vision_only"] = NFEAT_VISION, 1
            self.mt = MultiTracker(prm, self.max_sequences)
        return self.mt

    def start(self, slot, seq, n_frames=None):
        """a new sequence in `slot` (the slot's device-side local map is forgotten); its frame 0 initialises it"""
        mt = self._tracker(seq)
        assert slot not in self.lanes
        cls = _vision_lane() if self.vision else _LaneReplay
        r = cls(seq, self.S, max_local_points=self.max_local_points, **self.kw)
        n = n_frames or seq.n_frames
        r._n_run = n
        mt.reset_slot(slot)
        r.initialise()
        self.lanes[slot] = [r, 1, n]
        return r

    def step(self, order=None):
        """one call: the next frame of every running sequence (order: the slots in the order of the call's frames)"""
        order = sorted(self.lanes) if order is None else list(order)
        frames, ctxs = [], []
        t0 = time.perf_counter()
        for s in order:
            r, k, _ = self.lanes[s]
            r.before_frame(k)
            args, ctx = r.track_args(k)
            if self.into_planes:
                pl = self.mt.planes[s]
                pl[0][:], pl[1][:] = args["left"], args["right"]
                args["left"], args["right"] = pl[0], pl[1]
            frames.append((s, args))
            ctxs.append(ctx)
        res = self.mt.track(frames)
        self.stats["calls"] += 1
        self.stats["frames"] += len(frames)
        self.stats["ms_call"].append((float(res[0][0]["ms_host"]), float(res[0][0]["ms_gpu"])))
        self.stats["widened_calls"] += int(any(int(o["widened"]) for o, _ in res))
        for s, (o, v), ctx in zip(order, res, ctxs):
            lane = self.lanes[s]
            lane[0].apply_output(lane[1], o, v, ctx, t0)
            lane[1] += 1
            if lane[1] >= lane[2]:
                self.finished.append((s, lane[0]))
                del self.lanes[s]
        return res

    def run(self, seqs, n_frames=None):
        """every sequence in its own slot (0, 1, ...) until all have ended; the trajectories in the order of seqs"""
        ns = [n_frames] * len(seqs) if n_frames is None or np.isscalar(n_frames) else list(n_frames)
        reps = [self.start(s, seq, n) for s, (seq, n) in enumerate(zip(seqs, ns))]
        while self.lanes:
            self.step()
        return [np.array(r.traj, NAVSTATE_DTYPE) for r in reps]

    def close(self):
        if self.mt is not None:
            self.mt.close()
            self.mt = None


def _render_sequence(seed, n_frames):
    """(spawned process, CPU only) a replay.Sequence with its n_frames stereo pairs rendered; the scene itself stays
    behind (the images are all that is read of it)"""
    from . import replay
    seq = replay.Sequence(seed, n_frames)
    for k in range(n_frames):
        seq.images(k)
    seq.scene = None
    return seq


def make_sequences(seeds, n_frames, workers=8):
    """replay.Sequence(seed, n_frames) for every seed, rendered in spawned worker processes that never open the GPU"""
    import multiprocessing as mp
    seeds = [int(s) for s in seeds]
    with mp.get_context("spawn").Pool(max(1, min(workers, len(seeds)))) as pool:
        return pool.starmap(_render_sequence, [(s, n_frames) for s in seeds])
