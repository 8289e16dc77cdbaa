"""The batched visual-inertial PoseOptimization alone: ms per launch of vieo_pose_optimization_vio_batch_device_ex.
python tools/time_pose_batch.py [frames] [launches]     (default 2048 frames, 20 launches after 2 warm-up launches)

The frames are synthetic problems as the tests make them (synth_ba.make_vio_problem): 32 distinct ones -- 200..420
edges, every fourth with a free last state and a prior, every other with the marginalisation -- repeated over the
batch.  More than 256 frames take the one-wavefront-per-frame kernel; VIEO_POSE_THREADS=64|256 forces either form,
VIEO_LIB_PATH picks the build (A/B runs).  Also prints how many frames of the one-wavefront form a CU holds at a time
(vieo_debug_pose_vio_batch_residency; "n/a" for a build without that entry).
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vieo_slam_amd import synth_ba  # noqa: E402
from vieo_slam_amd._lib import DeviceBuffer, check, lib  # noqa: E402
from vieo_slam_amd.ba_types import VIO_FRAME_DTYPE, VIO_RESULT_DTYPE  # noqa: E402

N_PROTOS = 32


def protos():
    H0 = None
    out = []
    for i in range(N_PROTOS):
        kw = dict(n_obs=200 + 7 * i + (3 * i) % 11, compute_marg=(i % 2 == 0))
        if i % 4 == 1:  # last state free, with a marginal prior (30-dim system)
            if H0 is None:
                from vieo_slam_amd.optimizer import Optimizer
                F0, obs0, _ = synth_ba.make_vio_problem(900, compute_marg=True)
                H0 = Optimizer.PoseOptimizationVIO(F0, obs0)[0]["H_marg"].reshape(15, 15).copy()
            F1, _, _ = synth_ba.make_vio_problem(500 + i, **kw)
            nav_last = F1[0]["nav_last"].copy()
            nav_prior = nav_last.copy()
            nav_last["p"] += 0.004
            nav_last["v"] += 0.015
            kw["prior"] = (nav_prior, H0, nav_last)
        out.append(synth_ba.make_vio_problem(500 + i, **kw)[:2])
    return out


def residency():
    try:
        fn = lib().vieo_debug_pose_vio_batch_residency
    except AttributeError:
        return None
    fn.restype, fn.argtypes = ctypes.c_int, []
    return int(fn())


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    L = lib()
    P = protos()
    frames = np.zeros(B, VIO_FRAME_DTYPE)
    all_obs, begin = [], 0
    for i in range(B):
        F, obs = P[i % len(P)]
        frames[i] = F[0]
        frames[i]["base"]["obs_begin"] = begin
        begin += len(obs)
        all_obs.append(obs)
    obs = np.concatenate(all_obs)
    dF, dO = DeviceBuffer(frames.nbytes), DeviceBuffer(obs.nbytes)
    dU, dR = DeviceBuffer(len(obs)), DeviceBuffer(B * VIO_RESULT_DTYPE.itemsize)
    dF.upload(frames)
    dO.upload(obs)
    st, e0, e1 = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    check(L.vieo_stream_create(ctypes.byref(st)))
    check(L.vieo_event_create(ctypes.byref(e0)))
    check(L.vieo_event_create(ctypes.byref(e1)))
    call = lambda: check(L.vieo_pose_optimization_vio_batch_device_ex(dF.ptr, B, dO.ptr, dU.ptr, dR.ptr, 1, 1, st))
    for _ in range(2):
        call()
    check(L.vieo_stream_synchronize(st))
    check(L.vieo_event_record(e0, st))
    for _ in range(n):
        call()
    check(L.vieo_event_record(e1, st))
    check(L.vieo_stream_synchronize(st))
    ms = ctypes.c_float()
    check(L.vieo_event_elapsed_ms(e0, e1, ctypes.byref(ms)))
    res = dR.download(VIO_RESULT_DTYPE, (B,))
    r = residency()
    print({"frames": B, "launches": n, "ms_per_launch": round(ms.value / n, 4),
           "threads": os.environ.get("VIEO_POSE_THREADS") or ("64" if B > 256 else "256"),
           "frames_per_cu": "n/a" if r is None else r, "edges": int(len(obs)),
           "status_ok": int((res["base"]["status"] == 0).sum()), "lm_iterations": int(res["base"]["lm_iterations"].sum())})
    L.vieo_event_destroy(e0)
    L.vieo_event_destroy(e1)


if __name__ == "__main__":
    main()
