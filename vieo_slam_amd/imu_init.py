"""IMUInitialization::TryInitVIO (reference src/Odom/IMUInitialization.cpp:1068-1480) for a batch of sequences on the
C-ABI (vieo_imu_init): gyro bias, scale and gravity, accelerometer bias, and -- when the caller's gate is open -- the
scaled map with its NavStates.  `make_init_case` cuts such a problem out of a synthetic replay.Sequence."""
import numpy as np

from ._lib import check, lib
from .ba_types import IMU_PREINT_DTYPE, NAVSTATE_DTYPE
from .imu import IMU_NOISE_DTYPE, IMU_SAMPLE_DTYPE

MAX_KF, MAX_SEQ, MAX_SWEEPS = 512, 256, 30
OK, FEW_KF, FEW_EQUATIONS, DEGENERATE_GRAVITY = 0, 1, 2, 3
REF_G = 9.810  # IMUData::mdRefG

IMU_INIT_SEQ_DTYPE = np.dtype([("n_kf", "<i4"), ("n_kf_init", "<i4"), ("kf_first", "<i4"), ("point_first", "<i4"),
                               ("n_points", "<i4"), ("apply", "<i4"), ("Rcb", "<f8", 9), ("pcb", "<f8", 3),
                               ("ref_g", "<f8")], align=True)
IMU_INIT_POINT_DTYPE = np.dtype([("pos", "<f4", 3), ("max_dist", "<f4"), ("min_dist", "<f4")], align=True)
IMU_INIT_RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_eq_gyro", "<i4"), ("n_eq", "<i4"), ("inited", "<i4"),
                                  ("sweeps", "<i4", 2), ("bg", "<f8", 3), ("s_star", "<f8"), ("gw_star", "<f8", 3),
                                  ("w", "<f8", 4), ("RwI", "<f8", 9), ("s", "<f8"), ("dtheta", "<f8", 2), ("ba", "<f8", 3),
                                  ("w2", "<f8", 6), ("RwI_opt", "<f8", 9), ("gw", "<f8", 3)], align=True)
assert IMU_INIT_SEQ_DTYPE.itemsize == 128 and IMU_INIT_POINT_DTYPE.itemsize == 20 and IMU_INIT_RESULT_DTYPE.itemsize == 376


def extrinsics(Tbc):
    """(Rcb, pcb) as TryInitVIO forms them from Frame::mTbc: Rcb = Rbc^T, pcb = -Rcb pbc"""
    Tbc = np.asarray(Tbc, np.float64)
    Rcb = Tbc[:3, :3].T.copy()
    return Rcb, -Rcb @ Tbc[:3, 3]


def pack(cases):
    """The flat arrays of one vieo_imu_init call from the per-sequence cases (see try_init_vio)"""
    n_seq = len(cases)
    seqs = np.zeros(max(n_seq, 1), IMU_INIT_SEQ_DTYPE)
    kf0 = pt0 = 0
    Twc, ts, lists, pts, pre, prv = [], [], [], [], [], []
    stored = [c.get("preint") is not None for c in cases]
    if any(stored) and not all(stored):
        raise ValueError("stored pre-integrations: for every case or for none")
    for b, c in enumerate(cases):
        T = np.ascontiguousarray(c["Twc"], np.float64).reshape(-1, 12)
        n = len(T)
        if len(c["t"]) != n or len(c["samples"]) != n:
            raise ValueError("case %d: t and samples need one entry per key frame" % b)
        P = np.ascontiguousarray(c.get("points", np.zeros(0, IMU_INIT_POINT_DTYPE)), IMU_INIT_POINT_DTYPE).reshape(-1)
        q = seqs[b]
        q["n_kf"], q["n_kf_init"], q["kf_first"] = n, c.get("n_kf_init", n), kf0
        q["point_first"], q["n_points"], q["apply"] = pt0, len(P), int(c.get("apply", 1))
        q["Rcb"], q["pcb"] = np.asarray(c["Rcb"], np.float64).reshape(-1), np.asarray(c["pcb"], np.float64)
        q["ref_g"] = c.get("ref_g", REF_G)
        Twc.append(T), ts.append(np.asarray(c["t"], np.float64)), pts.append(P)
        lists += [np.ascontiguousarray(s, IMU_SAMPLE_DTYPE).reshape(-1) for s in c["samples"]]
        if stored[b]:
            pre.append(np.ascontiguousarray(c["preint"], IMU_PREINT_DTYPE).reshape(-1))
            prv.append(np.ascontiguousarray(c["preint_sigma_prv"], np.float64).reshape(-1, 81))
            if len(pre[-1]) != n or len(prv[-1]) != n:
                raise ValueError("case %d: preint and preint_sigma_prv need one entry per key frame" % b)
        kf0 += n
        pt0 += len(P)
    total_kf, total_pts = kf0, pt0
    Twc = np.concatenate(Twc) if Twc else np.zeros((0, 12))
    ts = np.concatenate(ts) if ts else np.zeros(0)
    first = np.concatenate([[0], np.cumsum([len(s) for s in lists])]).astype(np.int32)
    flat = np.concatenate(lists) if first[-1] else np.zeros(1, IMU_SAMPLE_DTYPE)
    pts = np.concatenate(pts) if total_pts else np.zeros(1, IMU_INIT_POINT_DTYPE)
    noise = np.ascontiguousarray(cases[0]["noise"], IMU_NOISE_DTYPE).reshape(1) if cases else np.zeros(1, IMU_NOISE_DTYPE)
    pre = np.concatenate(pre) if pre else None
    prv = np.concatenate(prv) if prv else None
    m = max(total_kf, 1)
    res = np.zeros(max(n_seq, 1), IMU_INIT_RESULT_DTYPE)
    Tcw, nav, nav_set = np.zeros((m, 12)), np.zeros(m, NAVSTATE_DTYPE), np.zeros(m, np.int32)
    pre_out, prv_out = np.zeros(m, IMU_PREINT_DTYPE), np.zeros((m, 81))
    pts_out = np.zeros(len(pts), IMU_INIT_POINT_DTYPE)
    return dict(seqs=seqs, n_seq=n_seq, total_kf=total_kf, Twc=Twc, t=ts, noise=noise, samples=flat, first=first, pre=pre,
                prv=prv, points=pts, total_points=total_pts, res=res, Tcw=Tcw, nav=nav, nav_set=nav_set, pre_out=pre_out,
                prv_out=prv_out, points_out=pts_out)


def call(pk):
    """vieo_imu_init on packed arrays (the outputs land in pk); returns the entry's return value"""
    ptr = lambda a: None if a is None else a.ctypes.data
    return lib().vieo_imu_init(ptr(pk["seqs"]), pk["n_seq"], pk["total_kf"], ptr(pk["Twc"]), ptr(pk["t"]), ptr(pk["noise"]),
                               ptr(pk["samples"]), ptr(pk["first"]), ptr(pk["pre"]), ptr(pk["prv"]), ptr(pk["points"]),
                               pk["total_points"], ptr(pk["res"]), ptr(pk["Tcw"]), ptr(pk["nav"]), ptr(pk["nav_set"]),
                               ptr(pk["pre_out"]), ptr(pk["prv_out"]), ptr(pk["points_out"]))


def try_init_vio(cases, raw=False):
    """cases: one dict per sequence --
      Twc [n_kf, 3, 4] float64 (the CV_32F mTwc widened), t [n_kf], samples: n_kf IMU_SAMPLE_DTYPE arrays (entry i: the
      interval i - 1 -> i; entry 0 empty), noise, Rcb, pcb, and optionally ref_g (9.810), n_kf_init (n_kf), apply (1),
      points (IMU_INIT_POINT_DTYPE[m]), preint + preint_sigma_prv (the stored pre-integrations [n_kf]; all cases or none).
    returns one dict per sequence: result (IMU_INIT_RESULT_DTYPE scalar), Tcw [n_kf, 3, 4], nav (NAVSTATE_DTYPE[n_kf]),
    nav_set [n_kf], preint (IMU_PREINT_DTYPE[n_kf]), sigma_prv [n_kf, 9, 9], points.  raw=True: (rc, list) without the
    check of the return value."""
    pk = pack(cases)
    rc = call(pk)
    if not raw:
        check(rc, "vieo_imu_init")
    out = []
    for b in range(pk["n_seq"]):
        q = pk["seqs"][b]
        k, n, p, npt = (int(q[f]) for f in ("kf_first", "n_kf", "point_first", "n_points"))
        out.append(dict(result=pk["res"][b].copy(), Tcw=pk["Tcw"][k:k + n].reshape(n, 3, 4).copy(), nav=pk["nav"][k:k + n].copy(),
                        nav_set=pk["nav_set"][k:k + n].copy(), preint=pk["pre_out"][k:k + n].copy(),
                        sigma_prv=pk["prv_out"][k:k + n].reshape(n, 9, 9).copy(), points=pk["points_out"][p:p + npt].copy()))
    return (rc, out) if raw else out


def make_init_case(seed, n_kf, step=10, s_true=1.0, Tbc=None, n_points=40, empty=(), **extra):
    """An initialisation problem from replay.Sequence(seed): key frames every `step` frames, the true Twb -> Twc
    re-expressed in key frame 0's camera frame (the reference's visual world; gravity is tilted there), positions divided
    by s_true (a visual map of unknown scale), poses rounded to float and widened again as mTwc would be, imu_between
    for the sample lists.  empty: key frames whose interval gets no samples (mdeltatij == 0).  The truth comes along:
    bg, ba, gw (in the visual world), s_true, the body velocities v [n_kf, 3] there."""
    from . import synth_ba
    from .replay import Sequence
    Tbc = np.asarray(synth_ba.EUROC_TBC if Tbc is None else Tbc, np.float64)
    seq = Sequence(seed, (n_kf - 1) * step + 2)
    Rbc, pbc = Tbc[:3, :3], Tbc[:3, 3]
    t = np.array([seq.time(k * step) for k in range(n_kf)])
    Rwc, pwc, vw = [], [], []
    for tk in t:
        R, p, v, _, _ = seq.state(tk)
        Rwc.append(R @ Rbc), pwc.append(p + R @ pbc), vw.append(v)
    R0, p0 = Rwc[0], pwc[0]
    Twc = np.zeros((n_kf, 3, 4))
    for k in range(n_kf):
        Twc[k, :, :3] = R0.T @ Rwc[k]
        Twc[k, :, 3] = R0.T @ (pwc[k] - p0) / s_true
    Twc = Twc.astype(np.float32).astype(np.float64)
    samples = [np.zeros(0, IMU_SAMPLE_DTYPE)]
    for k in range(1, n_kf):
        samples.append(np.zeros(0, IMU_SAMPLE_DTYPE) if k in empty else seq.imu_between(t[k - 1], t[k]).copy())
    rng = np.random.default_rng(seed + 7)
    pts = np.zeros(n_points, IMU_INIT_POINT_DTYPE)
    pts["pos"] = rng.uniform(-3, 3, (n_points, 3))
    pts["min_dist"] = rng.uniform(0.5, 1.5, n_points)
    pts["max_dist"] = pts["min_dist"] * rng.uniform(3, 8, n_points)
    Rcb, pcb = extrinsics(Tbc)
    case = dict(Twc=Twc, t=t, samples=samples, noise=seq.noise.copy(), Rcb=Rcb, pcb=pcb, ref_g=REF_G, points=pts,
                truth=dict(bg=seq.bg.copy(), ba=seq.ba.copy(), gw=R0.T @ synth_ba.GRAVITY, s=s_true,
                           v=np.array([R0.T @ v for v in vw])))
    case.update(extra)
    return case


def make_static_case(n_kf, dt=0.5, Tbc=None, **extra):
    """A body at rest with the identity pose, pcb = 0 and an accelerometer that reads (0, 0, 9.8): lambda is a zero column
    and gw* comes out along gI exactly, where TryInitVIO divides by zero (DEGENERATE_GRAVITY)."""
    t = 100.0 + dt * np.arange(n_kf)
    Twc = np.zeros((n_kf, 3, 4))
    Twc[:, :, :3] = np.eye(3)
    h = 1.0 / 200
    ts = t[0] - 2 * h + h * np.arange(int(round((n_kf - 1) * dt / h)) + 5)
    S = np.zeros(len(ts), IMU_SAMPLE_DTYPE)
    S["t"], S["a"] = ts, np.array([0, 0, 9.8])
    samples = [np.zeros(0, IMU_SAMPLE_DTYPE)]
    for k in range(1, n_kf):
        a = max(int(np.searchsorted(ts, t[k - 1], side="right")) - 1, 0)
        b = min(int(np.searchsorted(ts, t[k], side="left")), len(ts) - 1)
        samples.append(S[a:b + 1].copy())
    noise = np.zeros(1, IMU_NOISE_DTYPE)
    noise[0]["sigma_g"] = (np.eye(3) * 1e-6).reshape(-1)
    noise[0]["sigma_a"] = (np.eye(3) * 1e-4).reshape(-1)
    noise[0]["freq_ref"], noise[0]["dt_cov_noise_fixed"] = 200.0, 1
    case = dict(Twc=Twc, t=t, samples=samples, noise=noise, Rcb=np.eye(3), pcb=np.zeros(3), ref_g=REF_G)
    case.update(extra)
    return case
