"""Several live sequences tracked in lock step (vieo_tracker_multi_*, vieo_track_frames; csrc/tracker_multi.hip): one call
runs vieo_track_frame's chain once over one frame of each sequence, and every frame's output is byte for byte what a
vieo_tracker of its own returns for it."""
import os
import re
import subprocess

import numpy as np
import pytest

from vieo_slam_amd import replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEO_E_INVALID, VIEO_E_NO_DEVICE, VIEO_E_CAPACITY = -1, -2, -4
NEW_ENTRIES = ("vieo_tracker_multi_create", "vieo_tracker_multi_destroy", "vieo_tracker_multi_image_buffer",
               "vieo_tracker_multi_reset_slot", "vieo_track_frames", "vieo_track_local_queries_slot_batch_device")


# ---------------------------------------------------------------- CPU
def test_multi_header_and_python_mirror_agree(tmp_path):
    """A C program calls every new declaration (argument refusals: no device needed); the ctypes signatures bind and have
    the header's parameter counts."""
    src = tmp_path / "multi_abi.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "vieo_hot.h"
int main(void) {
  vieo_tracker_params P;
  memset(&P, 0, sizeof(P));
  vieo_tracker_multi* m = NULL;
  uint8_t* plane = NULL;
  int32_t slots[1] = {0};
  vieo_track_input in;
  vieo_track_output out;
  memset(&in, 0, sizeof(in));
  vieo_frustum_frame ff;
  memset(&ff, 0, sizeof(ff));
  int rc[6];
  rc[0] = vieo_tracker_multi_create(&m, &P, 4);  /* width 0 */
  rc[1] = vieo_tracker_multi_image_buffer(NULL, 0, 0, &plane);
  rc[2] = vieo_tracker_multi_reset_slot(NULL, 0);
  rc[3] = vieo_track_frames(NULL, 1, slots, &in, &out);
  rc[4] = vieo_track_local_queries_slot_batch_device(&ff, NULL, sizeof(vieo_vio_frame), NULL, sizeof(vieo_vio_result), 1,
                                                     NULL, NULL, NULL, NULL, NULL, 64, NULL, 0, 2.f, 0.f, NULL, NULL, NULL,
                                                     0, NULL, NULL);
  vieo_tracker_multi_destroy(NULL);
  rc[5] = m == NULL;
  printf("%d %d %d %d %d %d\n", rc[0], rc[1], rc[2], rc[3], rc[4], rc[5]);
  return 0;
}''')
    exe = tmp_path / "multi_abi"
    lib = os.path.join(ROOT, "vieo_slam_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + lib, "-lvieo_hot", "-Wl,-rpath," + lib])
    got = [int(x) for x in subprocess.check_output([str(exe)], timeout=120).split()]
    assert got == [VIEO_E_INVALID] * 5 + [1]
    from vieo_slam_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "vieo_hot.h")).read()
    for name in NEW_ENTRIES:
        assert getattr(L, name) is not None
        m = re.search(r"\b%s\(([^;]*)\);" % name, header)
        assert m, name
        n_params = len([p for p in m.group(1).split(",") if p.strip()])
        assert len(_lib._SIGS[name][1]) == n_params, name


def test_multi_create_checks_arguments_before_the_device():
    """max_sequences outside 1..256 and params vieo_tracker_create refuses: VIEO_E_INVALID with or without a device."""
    import ctypes
    from vieo_slam_amd import _lib
    from vieo_slam_amd.tracker import euroc_params
    L = _lib.lib()
    P = euroc_params()
    h = ctypes.c_void_p()
    for bad in (0, 257, -1):
        assert L.vieo_tracker_multi_create(ctypes.byref(h), P.ctypes.data, bad) == VIEO_E_INVALID
    for field, value in (("width", 0), ("height", -1), ("n_levels", 0), ("n_levels", 17), ("max_local_points", -1)):
        Q = P.copy()
        Q[0][field] = value
        assert L.vieo_tracker_multi_create(ctypes.byref(h), Q.ctypes.data, 4) == VIEO_E_INVALID, field
    assert L.vieo_tracker_multi_create(None, P.ctypes.data, 4) == VIEO_E_INVALID
    assert L.vieo_tracker_multi_create(ctypes.byref(h), None, 4) == VIEO_E_INVALID
    assert not h.value


# ---------------------------------------------------------------- GPU
_ARRAYS = ("keys", "desc", "uright", "depth", "point_ref", "outlier", "local_track_depth")
_NOT_COMPARED = _ARRAYS + ("key_group", "group_idx", "group_good", "group_p3d", "ms_gpu", "ms_host")


def _scalars(o):
    """the output record's bytes without its pointers and its two times"""
    from vieo_slam_amd.tracker import TRACK_OUTPUT_DTYPE
    r = np.zeros(1, TRACK_OUTPUT_DTYPE)
    r[0] = o
    for f in _NOT_COMPARED:
        r[0][f] = 0
    return r.tobytes()


def _record(rep, sample=()):
    """keeps every frame's output record (and the arrays of the sampled frames) as apply_output sees them"""
    rec = dict(out={}, arrays={})
    orig = rep.apply_output

    def apply_output(k, o, v, ctx, t0):
        rec["out"][k] = _scalars(o)
        if k in sample:
            rec["arrays"][k] = {n: np.array(v[n]).tobytes() for n in _ARRAYS}
        return orig(k, o, v, ctx, t0)
    rep.apply_output = apply_output
    return rec


def _solo(seq, n, stages, sample=(), vision=False, **kw):
    if vision:
        from vieo_slam_amd.replay_modes import VisionTrackerReplay as R
    else:
        from vieo_slam_amd.tracker import TrackerReplay as R
    rep = R(seq, stages, **kw)
    rec = _record(rep, sample)
    traj = rep.run(n)
    rep.close()
    return dict(traj=traj, stats=rep.stats, rec=rec)


def _traj(rep):
    from vieo_slam_amd.ba_types import NAVSTATE_DTYPE
    return np.array(rep.traj, NAVSTATE_DTYPE)


def _same(solo, rep, rec, n, what):
    t = _traj(rep)
    assert len(t) == n, what
    assert t.tobytes() == solo["traj"].tobytes(), what
    assert rep.stats["n_matches"] == solo["stats"]["n_matches"], what
    assert rep.stats["n_inliers"] == solo["stats"]["n_inliers"], what
    assert rep.stats["lba"] == solo["stats"]["lba"], what
    assert sorted(rec["out"]) == sorted(solo["rec"]["out"]), what
    for k in rec["out"]:
        assert rec["out"][k] == solo["rec"]["out"][k], (what, k)
    for k in rec["arrays"]:
        for name in _ARRAYS:
            assert rec["arrays"][k][name] == solo["rec"]["arrays"][k][name], (what, k, name)


@pytest.mark.gpu
@pytest.mark.parametrize("n_seq", [2, 8])
def test_gpu_lockstep_equals_solo(n_seq):
    """n sequences (different seeds, 40 frames, three local BAs each) in lock step: every trajectory, match and inlier
    count and output record equals the sequence's own TrackerReplay run byte for byte; the per-key arrays too on three
    sampled frames."""
    from vieo_slam_amd.tracker_multi import MultiTrackerReplay, make_sequences
    n, sample = 40, (1, 17, 39)
    seqs = make_sequences(range(21, 21 + n_seq), n)
    S = replay.HipStages()
    solo = [_solo(seq, n, S, sample) for seq in seqs]
    M = MultiTrackerReplay(S, n_seq)
    reps = [M.start(s, seq, n) for s, seq in enumerate(seqs)]
    recs = [_record(r, sample) for r in reps]
    while M.lanes:
        M.step()
    M.close()
    assert M.stats["calls"] == n - 1 and M.stats["frames"] == n_seq * (n - 1)
    for j in range(n_seq):
        assert solo[j]["stats"]["lba"] == 3
        _same(solo[j], reps[j], recs[j], n, "sequence %d" % j)


@pytest.mark.gpu
def test_gpu_lockstep_lengths_order_and_slot_reuse():
    """Sequences of 10 / 25 / 40 frames share one handle; the calls carry the running slots in reverse order; when the
    shortest ends its slot is reset and a new sequence starts there.  Every sequence equals its solo run."""
    from vieo_slam_amd.tracker_multi import MultiTrackerReplay, make_sequences
    lengths = [10, 25, 40, 22]
    seqs = make_sequences([31, 32, 33, 34], 40)
    S = replay.HipStages()
    solo = [_solo(seq, n, S) for seq, n in zip(seqs, lengths)]
    M = MultiTrackerReplay(S, 3)
    reps, recs = {}, {}
    for j in range(3):
        reps[j] = M.start(j, seqs[j], lengths[j])
        recs[j] = _record(reps[j])
    orders = []
    while M.lanes:
        order = sorted(M.lanes, reverse=True)
        orders.append(order)
        M.step(order)
        if 3 not in reps and not any(s == 0 for s in M.lanes):
            reps[3] = M.start(0, seqs[3], lengths[3])  # (start resets the slot: vieo_tracker_multi_reset_slot)
            recs[3] = _record(reps[3])
    M.close()
    assert all(o == sorted(o, reverse=True) for o in orders) and any(len(o) > 1 for o in orders)
    assert any(len(o) < 3 for o in orders) and M.finished[0][0] == 0 and M.finished[0][1] is reps[0]
    for j in range(4):
        _same(solo[j], reps[j], recs[j], lengths[j], "sequence %d" % j)


@pytest.mark.gpu
def test_gpu_lockstep_64_sequences():
    """64 sequences x 12 frames in one handle (the batched searches take their many-frame path): all equal their solo
    runs."""
    from vieo_slam_amd.tracker_multi import MultiTrackerReplay, make_sequences
    n, k = 12, 64
    seqs = make_sequences(range(100, 100 + k), n, workers=16)
    S = replay.HipStages()
    solo = [_solo(seq, n, S, sample=(11,)) for seq in seqs]
    M = MultiTrackerReplay(S, k)
    reps = [M.start(s, seq, n) for s, seq in enumerate(seqs)]
    recs = [_record(r, (11,)) for r in reps]
    while M.lanes:
        M.step()
    M.close()
    for j in range(k):
        _same(solo[j], reps[j], recs[j], n, "sequence %d" % j)


@pytest.mark.gpu
def test_gpu_lockstep_mixed_wider_window():
    """th_last = 0.12 (test_tracker.test_gpu_tracker_wider_window_branch): some calls hold widened and not widened frames
    together -- the tail runs again over all of them -- and all four sequences equal their solo runs."""
    from vieo_slam_amd.tracker_multi import MultiTrackerReplay, make_sequences
    n = 24
    seqs = make_sequences([3, 41, 42, 43], n)
    S = replay.HipStages()
    solo = [_solo(seq, n, S, sample=(5, 15), th_last=0.12) for seq in seqs]
    M = MultiTrackerReplay(S, 4, th_last=0.12)
    reps = [M.start(s, seq, n) for s, seq in enumerate(seqs)]
    recs = [_record(r, (5, 15)) for r in reps]
    mixed = 0
    while M.lanes:
        w = [int(o["widened"]) for o, _ in M.step()]
        mixed += 0 < sum(w) < len(w)
    M.close()
    assert mixed > 0, "no call mixed widened and not widened frames"
    assert sum(s["stats"]["widened"] for s in solo) > 0
    for j in range(4):
        _same(solo[j], reps[j], recs[j], n, "sequence %d" % j)


@pytest.mark.gpu
def test_gpu_lockstep_per_frame_preint_failure():
    """In one call one frame comes without IMU samples (VIEO_TRACK_PREINT_FAILED): its output and its neighbours' equal
    what the same inputs give through vieo_track_frame on trackers with the same history."""
    from vieo_slam_amd.tracker import TrackerReplay
    from vieo_slam_amd.tracker_multi import MultiTrackerReplay, make_sequences
    n_before = 5
    seqs = make_sequences([51, 52, 53], n_before + 1)
    S = replay.HipStages()
    solo = []
    for seq in seqs:
        r = TrackerReplay(seq, S)
        r.run(n_before)
        solo.append(r)
    M = MultiTrackerReplay(S, 3)
    reps = [M.start(s, seq, n_before + 1) for s, seq in enumerate(seqs)]
    for _ in range(n_before - 1):
        M.step()
    for r, q in zip(reps, solo):
        assert _traj(r).tobytes() == _traj(q).tobytes()
    k = n_before
    frames = []
    for s, r in enumerate(reps):
        args, _ = r.track_args(k)
        if s == 1:
            args["imu"] = args["imu"][:0]
        frames.append((s, args))
    got = [(_scalars(o), {n: np.array(v[n]).tobytes() for n in _ARRAYS}, int(o["status"])) for o, v in M.mt.track(frames)]
    M.close()
    for s, (_, args) in enumerate(frames):
        o, v = solo[s].trk.track(**args)
        assert got[s][0] == _scalars(o), s
        for name in _ARRAYS:
            assert got[s][1][name] == np.array(v[name]).tobytes(), (s, name)
        solo[s].close()
    assert [g[2] for g in got] == [0, 1, 0]  # VIEO_TRACK_PREINT_FAILED for the frame without samples only


@pytest.mark.gpu
def test_gpu_lockstep_vision_only():
    """Four vision-only sequences (params.vision_only, configs[0]) in lock step equal their VisionTrackerReplay runs."""
    from vieo_slam_amd.tracker_multi import MultiTrackerReplay, make_sequences
    n = 24
    seqs = make_sequences([61, 62, 63, 64], n)
    from vieo_slam_amd.replay_modes import HipVisionStages
    S = HipVisionStages()
    solo = [_solo(seq, n, S, sample=(3, 21), vision=True) for seq in seqs]
    M = MultiTrackerReplay(S, 4, vision=True)
    reps = [M.start(s, seq, n) for s, seq in enumerate(seqs)]
    recs = [_record(r, (3, 21)) for r in reps]
    while M.lanes:
        M.step()
    M.close()
    for j in range(4):
        assert solo[j]["stats"]["lba"] == 2
        _same(solo[j], reps[j], recs[j], n, "sequence %d" % j)


@pytest.mark.gpu
def test_gpu_lockstep_refusals_before_launch():
    """A duplicate slot, a slot >= max_sequences, next_left, use_prefetched, n = 0 (VIEO_E_INVALID) and too many IMU
    samples (VIEO_E_CAPACITY) are refused before anything runs: the sequences tracked behind them still equal their
    solo runs."""
    from vieo_slam_amd.imu import IMU_SAMPLE_DTYPE
    from vieo_slam_amd.tracker_multi import MultiTrackerReplay, make_sequences
    n = 14
    seqs = make_sequences([71, 72], n)
    S = replay.HipStages()
    solo = [_solo(seq, n, S) for seq in seqs]
    M = MultiTrackerReplay(S, 3)
    reps = [M.start(s, seq, n) for s, seq in enumerate(seqs)]
    recs = [_record(r) for r in reps]
    mt = M.mt
    refused = 0
    while M.lanes:
        k = reps[0].stats["frames"] + 1
        if k in (2, 11):  # (11: behind the first key frame's local BA, with a new local map pending)
            keep = []
            rec = [mt.record(s, keep, **r.track_args(k)[0]) for s, r in enumerate(reps)]
            rec = np.concatenate(rec)
            assert mt.call([0, 0], rec) == VIEO_E_INVALID
            assert mt.call([0, 3], rec) == VIEO_E_INVALID
            bad = rec.copy()
            bad[1]["next_left"] = bad[1]["left"]
            assert mt.call([0, 1], bad) == VIEO_E_INVALID
            bad = rec.copy()
            bad[0]["use_prefetched"] = 1
            assert mt.call([0, 1], bad) == VIEO_E_INVALID
            assert mt.call([], rec) == VIEO_E_INVALID
            many = np.zeros(600, IMU_SAMPLE_DTYPE)
            bad = rec.copy()
            bad[1]["imu"], bad[1]["n_imu"] = many.ctypes.data, len(many)
            assert mt.call([0, 1], bad) == VIEO_E_CAPACITY
            from vieo_slam_amd import _lib
            assert "slot 1" in _lib.lib().vieo_last_error().decode()
            refused += 1
        M.step()
    M.close()
    assert refused == 2
    for j in range(2):
        _same(solo[j], reps[j], recs[j], n, "sequence %d" % j)
