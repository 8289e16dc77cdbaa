"""Deterministic, named inputs of tests/test_device_algebra.py: for every family a few hundred seeded generic cases plus
the edges at which the lane functions change branch.  A case is (name, arrays...); a failure prints the name.
Every case is an input the library may legitimately receive: no NaN / Inf, no Pc.z = 0, no zero quaternion."""
import math

import numpy as np

from vieo_slam_amd import synth_ba
from vieo_slam_amd.ba_types import CAMERA_DTYPE

PI = math.pi
BELOW, ABOVE = np.nextafter(1e-5, 0.0), np.nextafter(1e-5, 1.0)
AXES = [("x", (1.0, 0.0, 0.0)), ("y", (0.0, 1.0, 0.0)), ("z", (0.0, 0.0, 1.0)),
        ("111", tuple(np.ones(3) / math.sqrt(3.0)))]
# rotation vectors by norm; "below" / "above" are the doubles next to 1e-5
ROT_NORMS = [("0", 0.0), ("1e-300", 1e-300), ("1e-9", 1e-9), ("0.99e-5", 0.99e-5), ("below-1e-5", BELOW),
             ("1e-5", 1e-5), ("above-1e-5", ABOVE), ("1.01e-5", 1.01e-5), ("1e-3", 1e-3), ("1", 1.0),
             ("pi-1e-9", PI - 1e-9), ("pi", PI), ("pi+1e-9", PI + 1e-9), ("2pi-1e-9", 2 * PI - 1e-9), ("7", 7.0),
             ("3", 3.0), ("pi-1e-6", PI - 1e-6)]          # the last two: JrInv


def _unit(rng, n=3):
    v = rng.normal(0, 1, n)
    return v / np.linalg.norm(v)


def _quat(rng):
    return _unit(rng, 4)


def rotvec_cases(n_generic=300, seed=101):
    out = []
    for nn, th in ROT_NORMS:
        for an, ax in AXES:
            out.append(("norm=%s/axis=%s" % (nn, an), th * np.array(ax)))
    rng = np.random.default_rng(seed)
    for k in range(n_generic):
        th = 10.0 ** rng.uniform(-8, 0) if k % 2 else rng.uniform(0.01, PI)
        out.append(("generic-%d" % k, th * _unit(rng)))
    return out


def quat_cases(n_generic=300, seed=102):
    """unit quaternions (to rounding) for so3_log_q and quat_to_R"""
    out = [("identity", np.array([1.0, 0, 0, 0])), ("minus-identity", np.array([-1.0, 0, 0, 0]))]
    edge = [("0.99e-5", 0.99e-5), ("below-1e-5", BELOW), ("1e-5", 1e-5), ("above-1e-5", ABOVE), ("1.01e-5", 1.01e-5)]
    for an, ax in (AXES[0], AXES[3]):
        ax = np.array(ax)
        for en, e in edge:
            for sn, s in (("+", 1.0), ("-", -1.0)):
                out.append(("n=%s/w%s/axis=%s" % (en, sn, an), np.concatenate([[s * math.sqrt(1 - e * e)], e * ax])))
                out.append(("w=%s%s/axis=%s" % (sn, en, an), np.concatenate([[s * e], math.sqrt(1 - e * e) * ax])))
        out.append(("w=0/axis=%s" % an, np.concatenate([[0.0], ax])))
    rng = np.random.default_rng(seed)
    for k in range(60):
        q = _quat(rng)
        q[0] = -abs(q[0])
        out.append(("w<0-generic-%d" % k, q))
    for k in range(n_generic):
        out.append(("generic-%d" % k, _quat(rng)))
    return out


def _rodrigues(axis, th):
    return synth_ba.quat_to_R(synth_ba.quat_from_rotvec(th * np.asarray(axis, float)))


def matrix_cases(n_generic=300, seed=103):
    """rotation matrices (row-major, orthonormal to rounding) for R_to_q"""
    rng = np.random.default_rng(seed)
    out = [("trace-positive-identity", np.eye(3)),
           ("trace-zero-120deg-about-111", np.array([[0.0, 0, 1], [1, 0, 0], [0, 1, 0]])),
           ("half-turn-about-x", np.diag([1.0, -1, -1])), ("half-turn-about-y", np.diag([-1.0, 1, -1])),
           ("half-turn-about-z", np.diag([-1.0, -1, 1])),
           ("half-turn-about-110", np.array([[0.0, 1, 0], [1, 0, 0], [0, 0, -1]])),
           ("half-turn-about-011", np.array([[-1.0, 0, 0], [0, 0, 1], [0, 1, 0]])),
           ("half-turn-about-101", np.array([[0.0, 0, 1], [0, -1, 0], [1, 0, 0]]))]
    for k in range(30):
        out.append(("179.999deg-random-axis-%d" % k, _rodrigues(_unit(rng), math.radians(179.999))))
    for an, ax in AXES[:3]:
        for deg in (100.0, 170.0):
            out.append(("%gdeg-about-%s" % (deg, an), _rodrigues(ax, math.radians(deg))))
    for k in range(n_generic):
        out.append(("generic-%d" % k, synth_ba.quat_to_R(_quat(rng))))
    return [(n, np.ascontiguousarray(R, np.float64).reshape(9)) for n, R in out]


def quat_pair_cases(n=300, seed=104):
    rng = np.random.default_rng(seed)
    return [("generic-%d" % k, _quat(rng), _quat(rng)) for k in range(n)]


def raw_quat_cases(n=300, seed=105):
    """quaternions of any length for q_norm"""
    rng = np.random.default_rng(seed)
    out = [("unit-w", np.array([1.0, 0, 0, 0])), ("two-z", np.array([0.0, 0, 0, 2.0]))]
    for k in range(n):
        out.append(("generic-%d" % k, _quat(rng) * 10.0 ** rng.uniform(-3, 3)))
    return out


# ---- B
def pose_inc_cases(n_generic=300, seed=201):
    """(name, pose (p, qw qx qy qz), increment (dp, dphi)) for inc_small_pr"""
    rng = np.random.default_rng(seed)
    out = []
    for nn, th in ROT_NORMS[:15]:
        for an, ax in AXES:
            out.append(("dphi-norm=%s/axis=%s" % (nn, an), np.concatenate([rng.uniform(-10, 10, 3), _quat(rng)]),
                        np.concatenate([rng.normal(0, 0.1, 3), th * np.array(ax)])))
    for k in range(n_generic):
        th = 10.0 ** rng.uniform(-8, -0.3)
        out.append(("generic-%d" % k, np.concatenate([rng.uniform(-10, 10, 3), _quat(rng)]),
                    np.concatenate([rng.normal(0, 0.1, 3), th * _unit(rng)])))
    return out


def state_inc_cases(n_generic=300, seed=202):
    """(name, state (p v q bg ba dbg dba: 22), dPVR (9), dBias (6)) for ns_inc"""
    rng = np.random.default_rng(seed)

    def state():
        return np.concatenate([rng.uniform(-10, 10, 3), rng.normal(0, 1, 3), _quat(rng), rng.normal(0, 0.01, 3),
                               rng.normal(0, 0.1, 3), rng.normal(0, 1e-3, 3), rng.normal(0, 1e-2, 3)])
    out = []
    for nn, th in ROT_NORMS[:15]:
        for an, ax in AXES:
            out.append(("dphi-norm=%s/axis=%s" % (nn, an), state(),
                        np.concatenate([rng.normal(0, 0.1, 3), rng.normal(0, 0.1, 3), th * np.array(ax)]),
                        rng.normal(0, 1e-3, 6)))
    for k in range(n_generic):
        th = 10.0 ** rng.uniform(-8, -0.3)
        out.append(("generic-%d" % k, state(),
                    np.concatenate([rng.normal(0, 0.1, 3), rng.normal(0, 0.1, 3), th * _unit(rng)]),
                    rng.normal(0, 1e-3, 6)))
    return out


# ---- C
def cameras():
    """(names, CAMERA_DTYPE array, image sizes): the rectified pinhole, the cameras of synth_ba.camera_rig("radtan")
    and ("kb8"), and Radtan cameras with 3, 4 and 6 radial coefficients"""
    rad, rad_size = synth_ba.camera_rig("radtan")
    kb8, kb8_size = synth_ba.camera_rig("kb8")
    cams = np.zeros(1 + len(rad) + len(kb8) + 4, CAMERA_DTYPE)
    names, sizes = ["pinhole"], [(synth_ba.W, synth_ba.H)]
    c = cams[0]
    c["model"], c["fx"], c["fy"], c["cx"], c["cy"] = 0, synth_ba.FX, synth_ba.FY, synth_ba.CX, synth_ba.CY
    c["Rcb"] = np.eye(3).reshape(-1)
    k = 1
    for i in range(len(rad)):
        cams[k] = rad[i]
        names.append("radtan%d-k2" % i), sizes.append(rad_size)
        k += 1
    for i in range(len(kb8)):
        cams[k] = kb8[i]
        names.append("kb8-%d" % i), sizes.append(kb8_size)
        k += 1
    # (radial polynomials that stay monotonic past the image corner, as a calibration's do)
    more = {3: [-0.2834, 0.0739, 0.0052], 4: [-0.2834, 0.0739, 0.0052, -0.0006],
            6: [-0.2834, 0.0739, 0.0052, -0.0006, 0.0001, -0.00001]}
    for nk, kk in more.items():
        cams[k] = rad[0]
        cams[k]["num_k"] = nk
        cams[k]["dist"] = 0
        cams[k]["dist"][:nk] = kk
        cams[k]["dist"][nk:nk + 2] = [0.00019359, 1.76187114e-05]
        names.append("radtan-k%d" % nk), sizes.append(rad_size)
        k += 1
    cams[k] = cams[0]                     # the rectified pinhole behind the body -> camera transform of the radtan rig
    cams[k]["Rcb"], cams[k]["tcb"] = rad[0]["Rcb"], rad[0]["tcb"]
    names.append("pinhole-body"), sizes.append((synth_ba.W, synth_ba.H))
    return names, cams, sizes


def camera_bf(cam):
    """bf of a camera of the table: the rectified pair's for the pinholes, 0 for a rig camera"""
    return float(np.float32(synth_ba.BF)) if int(cam["model"]) == 0 else 0.0


F1EM5 = float(np.float32(1e-5))


def project_cases(n_generic=90, seed=301):
    """(name, camera index, Pc)"""
    names, cams, sizes = cameras()
    rng = np.random.default_rng(seed)
    out = []
    for ci, cn in enumerate(names):
        c, (w, h) = cams[ci], sizes[ci]
        fx, fy, cx, cy = (float(c[t]) for t in ("fx", "fy", "cx", "cy"))
        for z in (0.3, 1.0, 200.0):
            out.append(("%s/on-axis-z=%g" % (cn, z), ci, np.array([0.0, 0.0, z])))
        if c["model"] == 2:
            # along an axis r is the coordinate itself, so the doubles next to 1e-5f sit on their side of the gate in
            # FP64 as in exact arithmetic; on a diagonal sqrt's rounding is as large as that step, so only 0.9x / 1.1x
            for rn, r in (("at", F1EM5), ("below", np.nextafter(F1EM5, 0.0)), ("above", np.nextafter(F1EM5, 1.0)),
                          ("0.9x", 0.9 * F1EM5), ("1.1x", 1.1 * F1EM5)):
                out.append(("%s/r-%s-1e-5f/along-x" % (cn, rn), ci, np.array([r, 0.0, 1.0])))
                out.append(("%s/r-%s-1e-5f/along-y" % (cn, rn), ci, np.array([0.0, -r, 0.5])))
                if rn in ("0.9x", "1.1x"):
                    out.append(("%s/r-%s-1e-5f/diagonal" % (cn, rn), ci, np.array([r * 0.6, -r * 0.8, 2.0])))
            for deg in (1.0, 45.0, 89.0, 91.0, 120.0):       # beyond 90 degrees z < 0
                for az in (0.0, 0.7, 2.0, 4.0):
                    t = math.radians(deg)
                    d = rng.uniform(0.3, 200.0)
                    out.append(("%s/field-angle-%gdeg/az=%g" % (cn, deg, az), ci,
                                d * np.array([math.sin(t) * math.cos(az), math.sin(t) * math.sin(az), math.cos(t)])))
            for k in range(n_generic):
                t, az, d = rng.uniform(0, math.radians(110)), rng.uniform(0, 2 * PI), 10.0 ** rng.uniform(-0.5, 2.3)
                out.append(("%s/generic-%d" % (cn, k), ci,
                            d * np.array([math.sin(t) * math.cos(az), math.sin(t) * math.sin(az), math.cos(t)])))
        else:
            # r up to the image corner (one pixel inside: a point that lands on pixel 0 exactly is a difference of equal
            # terms, whose float rounding no FP64 evaluation can be asked to reproduce)
            for un, u, v in (("tl", 1, 1), ("tr", w - 1, 1), ("bl", 1, h - 1), ("br", w - 1, h - 1)):
                for z in (0.3, 200.0):
                    out.append(("%s/corner-%s-z=%g" % (cn, un, z), ci, z * np.array([(u - cx) / fx, (v - cy) / fy, 1.0])))
            for k in range(n_generic):
                u, v, z = rng.uniform(0, w), rng.uniform(0, h), 10.0 ** rng.uniform(-0.5, 2.3)
                out.append(("%s/generic-%d" % (cn, k), ci, z * np.array([(u - cx) / fx, (v - cy) / fy, 1.0])))
    return out


def unproject_cases(n_generic=60, seed=302):
    """(name, camera index, pixel (float32 values)) for cam_unproject"""
    names, cams, sizes = cameras()
    rng = np.random.default_rng(seed)
    out = []
    for ci, cn in enumerate(names):
        c, (w, h) = cams[ci], sizes[ci]
        cx, cy, fx = float(c["cx"]), float(c["cy"]), float(c["fx"])
        out.append(("%s/principal-point" % cn, ci, (cx, cy)))
        for un, u, v in (("tl", 0, 0), ("tr", w - 1, 0), ("bl", 0, h - 1), ("br", w - 1, h - 1)):
            out.append(("%s/corner-%s" % (cn, un), ci, (u, v)))
        if c["model"] == 2:
            out.append(("%s/next-to-principal-point" % cn, ci, (float(np.nextafter(np.float32(cx), np.float32(1e9))), cy)))
            for f in (0.999, 1.001, 1.2):
                out.append(("%s/thetad=%g-half-pi" % (cn, f), ci, (cx + f * PI / 2 * fx, cy)))
        for k in range(n_generic):
            out.append(("%s/generic-%d" % (cn, k), ci, (rng.uniform(0, w - 1), rng.uniform(0, h - 1))))
    return [(n, ci, np.array(uv, np.float32).astype(np.float64)) for n, ci, uv in out]


def pinhole_unproject_cases(n_generic=20, seed=303):
    """(name, camera index, pixel (any double)) for unproject_pinhole"""
    names, cams, sizes = cameras()
    rng = np.random.default_rng(seed)
    out = []
    for ci, cn in enumerate(names):
        out.append(("%s/principal-point" % cn, ci, np.array([float(cams[ci]["cx"]), float(cams[ci]["cy"])])))
        for k in range(n_generic):
            out.append(("%s/generic-%d" % (cn, k), ci, rng.uniform(0, 1, 2) * np.array(sizes[ci], float)))
    return out


# ---- G
POOL_T, POOL_N, POOL_BLOCKS = 256, 28, 16


def reduction_pool(seed=701):
    """[2][16][256][28]: blocks 0..5 mixed signs over 1e-8 .. 1e8; 6 all zero; 7..14 one non-zero thread, in the 32-thread
    part 0..7 in turn; 15 integers.  Data set 1 of block b is data set 0 of block (b + 1) % 16, so that a function's
    second call can be compared with another block's first call on the same data."""
    rng = np.random.default_rng(seed)
    d0 = np.zeros((POOL_BLOCKS, POOL_T, POOL_N))
    kinds = []
    for b in range(POOL_BLOCKS):
        if b < 6:
            d0[b] = rng.choice([-1.0, 1.0], (POOL_T, POOL_N)) * 10.0 ** rng.uniform(-8, 8, (POOL_T, POOL_N))
            kinds.append("mixed-%d" % b)
        elif b == 6:
            kinds.append("all-zero")
        elif b < 15:
            part = b - 7
            d0[b, part * 32 + int(rng.integers(0, 32))] = rng.normal(0, 1, POOL_N) * 10.0 ** rng.uniform(-8, 8, POOL_N)
            kinds.append("one-thread-in-part-%d" % part)
        else:
            d0[b] = rng.integers(-2 ** 20, 2 ** 20, (POOL_T, POOL_N)).astype(np.float64)
            kinds.append("integers")
    return np.stack([d0, np.roll(d0, -1, axis=0)]), kinds


# ---- E
def _state(rng, q=None):
    return np.concatenate([rng.uniform(-10, 10, 3), rng.normal(0, 1, 3), _quat(rng) if q is None else q,
                           rng.normal(0, 0.01, 3), rng.normal(0, 0.1, 3), np.zeros(6)])


def _imu_case(rng, dt, Rij, res_R, bias, gw=(0.0, 0.0, -9.81), w_norm=None):
    """a pre-integrated measurement (61 doubles in vieo_imu_preint's order), gravity, and two states whose rotation
    residual is about res_R and whose position / velocity residuals are a few millimetres; w_norm: the gyroscope bias
    correction is scaled so that |JgR dbg| is this (the random draws are the same with and without)"""
    gw = np.array(gw)
    si = _state(rng)
    if bias:
        si[16:19], si[19:22] = rng.normal(0, 1e-3, 3), rng.normal(0, 1e-3, 3)
    Ri = synth_ba.quat_to_R(si[6:10])
    vij, pij = rng.normal(0, 2, 3) * dt, rng.normal(0, 1, 3) * dt * dt
    JgR, Jgv, Jav = rng.normal(0, 1, (3, 3)) * dt, rng.normal(0, 1, (3, 3)) * dt * dt, -np.eye(3) * dt
    Jgp, Jap = rng.normal(0, 1, (3, 3)) * dt ** 3, -np.eye(3) * dt * dt / 2 + rng.normal(0, 1e-3, (3, 3))
    if w_norm is not None:
        si[16:19] *= w_norm / np.linalg.norm(JgR @ si[16:19])
    dbg, dba = si[16:19], si[19:22]
    Rc = Rij @ synth_ba.so3_exp(JgR @ dbg)
    Rj = Ri @ Rc @ synth_ba.so3_exp(np.asarray(res_R, float))
    sj = _state(rng, synth_ba._R_to_quat(Rj))
    sj[3:6] = si[3:6] + gw * dt + Ri @ (vij + Jgv @ dbg + Jav @ dba) + rng.normal(0, 2e-3, 3)
    sj[0:3] = si[0:3] + si[3:6] * dt + gw * dt * dt / 2 + Ri @ (pij + Jgp @ dbg + Jap @ dba) + rng.normal(0, 2e-3, 3)
    M = np.concatenate([[dt], Rij.reshape(-1), vij, pij, JgR.reshape(-1), Jgv.reshape(-1), Jav.reshape(-1),
                        Jgp.reshape(-1), Jap.reshape(-1)])
    return M, gw, si, sj


def imu_cases(n_generic=100, seed=501):
    """(name, measurement (61), gw, state i (22), state j (22), idR): every case in the PVR (idR = 6) and the PRV
    (idR = 3) ordering"""
    rng = np.random.default_rng(seed)
    base = []
    for dt in (0.05, 0.5):
        for bn, bias in (("zero-bias", False), ("bias-1e-3", True)):
            for an, ax in AXES[:3]:
                for rn, ang in (("small", 0.02), ("100deg", math.radians(100.0)), ("170deg", math.radians(170.0))):
                    base.append(("dt=%g/%s/Rij-%s-about-%s" % (dt, bn, rn, an),
                                 _imu_case(rng, dt, _rodrigues(ax, ang), rng.normal(0, 1e-2, 3), bias)))
    base.append(("residual-below-1e-5", _imu_case(rng, 0.05, _rodrigues(_unit(rng), 0.05), 1e-7 * _unit(rng), True)))
    base.append(("residual-3rad", _imu_case(rng, 0.05, _rodrigues(_unit(rng), 0.05), 3.0 * _unit(rng), True)))
    # a clean measurement: every term is exactly representable, so the residual is exactly zero
    dt, g = 0.5, np.array([0.0, 0.0, -9.8125])
    si = np.zeros(22)
    si[6] = 1.0
    M = np.concatenate([[dt], np.eye(3).reshape(-1), -g * dt, -g * (dt * dt / 2), np.zeros(45)])
    base.append(("clean-measurement", (M, g, si, si.copy())))
    for k in range(n_generic):
        ang = rng.uniform(0, 2.0)
        base.append(("generic-%d" % k, _imu_case(rng, rng.choice([0.05, 0.5]), _rodrigues(_unit(rng), ang),
                                                  rng.normal(0, 1e-2, 3), k % 2 == 0)))
    out = []
    for name, (M, gw, si, sj) in base:
        out.append((name + "/PVR", M, gw, si, sj, 6))
        out.append((name + "/PRV", M, gw, si, sj, 3))
    return out


def enc_cases(n_generic=200, seed=502):
    """(name, state i, state j, measurement (dphi, dp), qRbe, pbe)"""
    rng = np.random.default_rng(seed)
    qbe = synth_ba._R_to_quat(synth_ba.ENC_RBE)
    pbe = np.array([0.1, -0.02, 0.05])
    out = []

    def case(name, res_R, move):
        si = _state(rng)
        Ri = synth_ba.quat_to_R(si[6:10])
        Rj = Ri @ synth_ba.so3_exp(np.asarray(move, float))
        sj = _state(rng, synth_ba._R_to_quat(Rj))
        sj[0:3] = si[0:3] + rng.normal(0, 0.3, 3)
        Rbe = synth_ba.ENC_RBE
        Re = Rbe.T @ Ri.T @ Rj @ Rbe
        meas_R = synth_ba.so3_log_np(Re @ synth_ba.so3_exp(-np.asarray(res_R, float)))
        dp = Rbe.T @ (Ri.T @ (sj[0:3] - si[0:3]) - pbe + Ri.T @ Rj @ pbe)
        out.append((name, si, sj, np.concatenate([meas_R, dp + rng.normal(0, 1e-3, 3)]), qbe, pbe))
    case("residual-below-1e-5", 1e-7 * _unit(rng), 0.1 * _unit(rng))
    case("residual-3rad", 3.0 * _unit(rng), 0.1 * _unit(rng))
    case("no-motion", 1e-3 * _unit(rng), np.zeros(3))
    for k in range(n_generic):
        case("generic-%d" % k, rng.normal(0, 1e-2, 3), rng.uniform(0, 1.0) * _unit(rng))
    return out


# ---- D
def visual_cases(n_generic=200, seed=401):
    """(name, index of the frame's camera, first camera of the rig, pose (p, q), observation (Xw, u, v, ur, inv_sigma2:
    float values), flags, Huber width).  The rigs are four consecutive cameras of the table: from 0 (pinhole, two Radtan,
    one KB8) and from 3 (four KB8)."""
    names, cams, sizes = cameras()
    rng = np.random.default_rng(seed)
    body = names.index("pinhole-body")
    out = []

    def case(name, c0, rig, ci, depth, stereo):
        c = cams[c0]
        p, q = rng.uniform(-10, 10, 3), _quat(rng)
        Rwb, Rcb = synth_ba.quat_to_R(q), c["Rcb"].reshape(3, 3)
        Xc = depth * np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.3, 0.3), 1.0])
        Xw = (Rwb @ (Rcb.T @ (Xc - c["tcb"])) + p).astype(np.float32).astype(np.float64)
        Pc = Rcb @ Rwb.T @ (Xw - p) + c["tcb"]
        level = int(rng.integers(0, 8))
        u = float(c["fx"]) * Pc[0] / Pc[2] + float(c["cx"]) + rng.normal(0, 1.2 ** level)
        v = float(c["fy"]) * Pc[1] / Pc[2] + float(c["cy"]) + rng.normal(0, 1.2 ** level)
        ur = u - camera_bf(c) / Pc[2] + rng.normal(0, 1.2 ** level) if stereo else -1.0
        ob = np.array([Xw[0], Xw[1], Xw[2], u, v, ur, 1.0 / 1.2 ** (2 * level)], np.float32).astype(np.float64)
        out.append((name, c0, rig, np.concatenate([p, q]), ob, (ci << 8) | 1, math.sqrt(7.815 if stereo else 5.991)))
    for c0, cn in ((0, "Rcb=identity"), (body, "Rcb=body")):
        for rig in (0, 3):
            for ci in range(4):
                for depth in (0.3, 5.0, 200.0):
                    for stereo in (False, True):
                        case("%s/rig-from-%d/camera-%d/depth=%g/%s" % (cn, rig, ci, depth, "stereo" if stereo else "mono"),
                             c0, rig, ci, depth, stereo)
    for k in range(n_generic):
        case("generic-%d" % k, (0, body)[k % 2], (0, 3)[(k // 2) % 2], int(rng.integers(0, 4)),
             10.0 ** rng.uniform(-0.5, 2.3), bool(rng.random() < 0.7))
    return out


def huber_cases(n_generic=200, seed=402):
    """(name, e, delta, dsqr)"""
    rng = np.random.default_rng(seed)
    out = []
    for dn, d in (("mono", math.sqrt(5.991)), ("stereo", math.sqrt(7.815)), ("encoder", float(np.float32(math.sqrt(12.592))))):
        q = d * d
        for en, e in (("e=0", 0.0), ("e=dsqr", q), ("e-below-dsqr", np.nextafter(q, 0.0)), ("e-above-dsqr", np.nextafter(q, 1e9)),
                      ("e=dsqr/1000", q / 1000), ("e=10dsqr", 10 * q)):
            out.append(("%s/%s" % (dn, en), e, d, q))
    for k in range(n_generic):
        d = math.sqrt(5.991)
        out.append(("generic-%d" % k, 10.0 ** rng.uniform(-3, 3), d, d * d))
    return out


# ---- F
def _look(rng, centre, target, roll=0.0):
    """Tcw (3 x 4) of a camera at `centre` whose optical axis points at `target`"""
    z = (target - centre) / np.linalg.norm(target - centre)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    Rcw = np.stack([x, y, z]) @ np.eye(3)
    if roll:
        Rcw = synth_ba.so3_exp(np.array([0.0, 0.0, roll])) @ Rcw
    return np.hstack([Rcw, (-Rcw @ centre)[:, None]])


def tri_cases(N, oracle, n_generic=100, seed=601):
    """(name, slots, thresh, just_check_p3d, x3d) for triangulate_matches_world<N>.  A slot is (on, camera index,
    Tcw[3, 4], n (UnProject of the key point by the FP64 oracle), u, v, sigma2, uright, bf), the floats as float32."""
    names, cams, sizes = cameras()
    rng = np.random.default_rng(seed + N)
    f = np.float32
    TH = float(f(1. - 1e-6))
    pool = [names.index(k) for k in ("pinhole", "radtan0-k2", "radtan1-k2", "kb8-0", "kb8-1", "kb8-2")]
    off = (False, 0, np.hstack([np.eye(3), np.zeros((3, 1))]), np.array([0.0, 0.0, 1.0]), f(0), f(0), f(1), f(-1), f(0))
    out = []

    def observe(ci, T, X, noise=0.3, stereo=False):
        c = cams[ci]
        Pc = T[:, :3] @ X + T[:, 3]
        uv = np.array(synth_ba.project_camera(c, Pc)) + rng.normal(0, noise, 2)
        uv = uv.astype(np.float32)
        nP = oracle.cam_unproject(c, uv)
        bf = f(synth_ba.BF)
        ur = f(uv[0] - bf / f(Pc[2]) + rng.normal(0, noise)) if stereo else f(-1)
        return (True, ci, T, nP, uv[0], uv[1], f(1.44), ur, bf if stereo else f(0))

    def scene(k, depth=4.0, baseline=0.5, **kw):
        X = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.3, 0.3), depth])
        return X, [observe(pool[int(rng.integers(0, len(pool)))],
                           _look(rng, np.array([baseline * (i - (k - 1) / 2), rng.uniform(-0.05, 0.05), 0.0]), X + rng.normal(0, 0.2 * depth / 4, 3)),
                           X, **kw) for i in range(k)]

    def place(slots, pattern):
        it = iter(slots)
        return [next(it) if p else off for p in pattern]

    def add(name, slots, thresh=TH, just=False, x3d=(0.0, 0.0, 0.0)):
        assert len(slots) == N
        out.append((name, slots, thresh, just, np.asarray(x3d, np.float64)))
    full = lambda k: [1] * k + [0] * (N - k)
    for k in range(2, N + 1):
        X, s = scene(k)
        add("%d-observations" % k, place(s, full(k)))
    if N >= 4:
        for pn, pat in (("front", [0] * (N - 3) + [1, 1, 1]), ("middle", [1, 1] + [0] * (N - 3) + [1]), ("end", [1, 1, 1] + [0] * (N - 3)),
                        ("scattered", ([0, 1, 0, 0, 1, 0, 1, 0] + [0] * N)[:N])):
            X, s = scene(3)
            add("empty-slots-at-the-%s" % pn, place(s, pat))
        X, s = scene(2)
        add("two-identical-rays-and-a-third", place([s[0], s[0], s[1]], full(3)))
    X, s = scene(2, baseline=0.5)
    add("parallax-enough", place(s, full(2)))
    X, s = scene(2, depth=150.0, baseline=0.01, noise=0.0)          # rays 7e-5 rad apart: the float cosine is 1
    add("parallax-too-small", place(s, full(2)))
    add("parallax-gate-off/thresh=1", place(s, full(2)), thresh=1.0)
    X, s = scene(2)
    Cb = np.array([0.3, 0.0, 2 * X[2]])
    Tb = _look(rng, Cb, np.array([0.3, 0.0, 3 * X[2]]))          # looks away from the point: it sees the point's mirror
    s[1] = observe(s[1][1], Tb, 2 * Cb - X, noise=0.0)           # image through its centre, on the same line
    add("point-behind-one-camera", place(s, full(2)), thresh=1.0)
    X, s = scene(2, stereo=True)
    add("stereo-slots", place(s, full(2)))
    X, s = scene(2, stereo=True)
    s[0] = s[0][:7] + (np.float32(s[0][7] + 40.0),) + s[0][8:]
    add("stereo-slot-right-image-off", place(s, full(2)))
    X, s = scene(2)
    add("just_check_p3d/the-point", place(s, full(2)), thresh=1.0, just=True, x3d=X)
    add("just_check_p3d/a-wrong-point", place(s, full(2)), thresh=1.0, just=True, x3d=X + np.array([0.5, 0.0, 0.0]))
    X, s = scene(2, noise=8.0)
    add("reprojection-too-large", place(s, full(2)))
    # parallel rays along z from identity rotations: column 2 of A is exactly zero, the null vector is (0, 0, 1, 0)
    I = lambda tx: np.hstack([np.eye(3), np.array([[tx], [0.0], [0.0]])])
    pin = names.index("pinhole")
    pp = (np.float32(cams[pin]["cx"]), np.float32(cams[pin]["cy"]))
    ray = lambda tx: (True, pin, I(tx), np.array([0.0, 0.0, 1.0]), pp[0], pp[1], f(1.44), f(-1), f(0))
    add("point-at-infinity/x4[3]=0", place([ray(0.0), ray(-0.5)], full(2)), thresh=1.0)
    for k in range(n_generic):
        n_on = int(rng.integers(2, N + 1))
        X, s = scene(n_on, depth=10.0 ** rng.uniform(-0.3, 1.5), baseline=rng.uniform(0.1, 1.0), stereo=bool(k % 5 == 0))
        pat = np.zeros(N, int)
        pat[rng.choice(N, n_on, replace=False)] = 1
        add("generic-%d" % k, place(s, list(pat)))
    return out


def null_cases(M, oracle, seed=602):
    """(name, A[M, 4], well-defined): the DLT systems of the triangulation cases with 2 * on-slots <= M (zero rows for
    the rest) and matrices that make null_vector4 skip rotations (g == 0) or have no single null vector"""
    out = []
    for N in (2, 8):
        for name, slots, *_ in tri_cases(N, oracle, n_generic=60):
            on = [s for s in slots if s[0]]
            if 2 * N != M and not (M == 8 and N == 8 and len(on) <= 4):
                continue
            A = np.zeros((M, 4))
            rows = slots if 2 * N == M else on
            for i, s in enumerate(rows):
                if s[0]:
                    A[2 * i] = s[3][0] * s[2][2] - s[2][0]
                    A[2 * i + 1] = s[3][1] * s[2][2] - s[2][1]
            out.append(("tri%d/%s" % (N, name), A, "x4[3]=0" not in name))
    D = np.zeros((M, 4))
    D[0, 0], D[1, 1], D[2, 2], D[3, 3] = 3.0, 2.0, 1.0, 0.5
    out.append(("orthogonal-columns/g=0-everywhere", D, True))
    D2 = D.copy()
    D2[3, 3] = 0.0
    out.append(("zero-column", D2, True))
    rng = np.random.default_rng(seed + M)
    B = rng.normal(0, 1, (M, 2)) @ rng.normal(0, 1, (2, 4))
    out.append(("rank-2/no-single-null-vector", B, False))
    return out


# ---- the fast forms of the VIO pose kernel (csrc/vio_fast_device.h), tests/test_vio_fast_algebra.py
HALF_BELOW, HALF_ABOVE = float(np.nextafter(0.5, 0.0)), float(np.nextafter(0.5, 1.0))
LOG_EDGE = 2 * math.atan(0.25)      # tan^2 of the half angle = 1 / 16: 0.48996 rad


def vio_rotvec_cases(n_generic=200, seed=801):
    """(name, w, inside |w|^2 < 1 / 4?) for so3_exp_unit / so3_Jr_unit.  The edge is met along one axis, where
    |w|^2 = w_k^2 is one rounded product whatever the compiler fuses: |w| one ulp below 0.5, 0.5 and one ulp above."""
    out = [("u=0", np.zeros(3), True), ("u=1e-20", np.array([0.0, 1e-10, 0.0]), True)]
    for an, ax in AXES[:3]:
        ax = np.array(ax)
        out += [("|w|-one-ulp-below-0.5/axis=%s" % an, HALF_BELOW * ax, True), ("|w|=0.5/axis=%s" % an, 0.5 * ax, False),
                ("|w|-one-ulp-above-0.5/axis=%s" % an, HALF_ABOVE * ax, False)]
    a111 = np.array(AXES[3][1])
    out += [("u=0.3/axis=111", math.sqrt(0.3) * a111, False), ("u=3/axis=111", math.sqrt(3.0) * a111, False)]
    rng = np.random.default_rng(seed)
    for k in range(n_generic):
        th = 10.0 ** rng.uniform(-8, math.log10(0.499)) if k % 2 else rng.uniform(0.01, 0.499)
        out.append(("generic-%d" % k, th * _unit(rng), True))
    return out


def _log_edge_pair(w):
    """the adjacent doubles x_in < x_out with fl(x x) < fl(w w) / 16 for the first only (q = (w, x, 0, 0))"""
    lim = 0.0625 * (w * w)
    x = 0.25 * abs(w)
    while x * x < lim:
        x = float(np.nextafter(x, 1.0))
    while not x * x < lim:
        x = float(np.nextafter(x, 0.0))
    return x, float(np.nextafter(x, 1.0))


def vio_quat_cases(n_generic=200, seed=802):
    """(name, q, so3_log_unit's domain test passes?, |q|^2 - 1 as built or None) for q_renorm, so3_log_unit and
    so3_JrInv_g.  Every quaternion but the `norm` cases is unit to rounding."""
    out = [("n2=0", np.array([1.0, 0, 0, 0]), True, None), ("n2=0/w<0", np.array([-1.0, 0, 0, 0]), True, None),
           ("w=0", np.array([0.0, 1.0, 0, 0]), False, None)]
    for sn, s in (("w>0", 1.0), ("w<0", -1.0)):
        w = s * math.cos(LOG_EDGE / 2)
        x_in, x_out = _log_edge_pair(w)
        out += [("one-ulp-inside-1/16/%s" % sn, np.array([w, x_in, 0, 0]), True, None),
                ("one-ulp-outside-1/16/%s" % sn, np.array([w, x_out, 0, 0]), False, None)]
    rng = np.random.default_rng(seed)
    q0 = synth_ba.quat_from_rotvec(0.2 * _unit(rng))
    for en, e in (("1e-16", 1e-16), ("1e-8", 1e-8), ("0.99e-5", 0.99e-5), ("1.01e-5", 1.01e-5)):
        for sn, s in (("+", 1.0), ("-", -1.0)):
            out.append(("norm/|q|^2-1=%s%s" % (sn, en), q0 * math.sqrt(1 + s * e), True, s * e))
    for k in range(30):
        out.append(("w<0-inside-%d" % k, -synth_ba.quat_from_rotvec(rng.uniform(0.01, 0.48) * _unit(rng)), True, None))
    for k in range(20):
        out.append(("outside-%d" % k, synth_ba.quat_from_rotvec(rng.uniform(0.5, 3.1) * _unit(rng)), False, None))
    for k in range(n_generic):
        th = 10.0 ** rng.uniform(-8, math.log10(0.489)) if k % 2 else rng.uniform(0.01, 0.489)
        out.append(("generic-%d" % k, synth_ba.quat_from_rotvec(th * _unit(rng)), True, None))
    return out


def vio_rcp_cases(n=100, seed=803):
    rng = np.random.default_rng(seed)
    out = [("1", 1.0), ("3", 3.0), ("-7", -7.0), ("2^-100", 2.0 ** -100), ("1e30", 1e30)]
    return out + [("generic-%d" % k, float(rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(-12, 12))) for k in range(n)]


def vio_imu_cases(seed=811):
    """(name, measurement, gw, state i, state j, ok?, w_small?): the PVR cases of imu_cases and the edges of
    imu_error_rot's domains.  ok carries w_small on, so w_small = False with ok = True cannot be."""
    out = []
    for n, M, gw, si, sj, idR in imu_cases():
        if idR == 6:
            out.append((n[:-4], M, gw, si, sj, "residual-3rad" not in n, True))
    rng = np.random.default_rng(seed)

    def add(name, res, ok, w_small, w_norm=None, qs=1.0):
        M, gw, si, sj = _imu_case(rng, 0.05, _rodrigues(_unit(rng), 0.3), res * _unit(rng), True, w_norm=w_norm)
        si[6:10] *= qs
        out.append((name, M, gw, si, sj, ok, w_small))
    add("residual-0.4895rad", 0.4895, True, True)
    add("residual-0.4905rad", 0.4905, False, True)
    add("w=0.499/residual-small", 0.01, True, True, 0.499)
    add("w=0.501/residual-small", 0.01, False, False, 0.501)
    add("w=0.499/residual-0.4905rad", 0.4905, False, True, 0.499)
    add("w=0.501/residual-0.4905rad", 0.4905, False, False, 0.501)
    add("state-quaternion-unit-to-1e-7", 0.01, True, True, None, 1 + 1e-7)
    add("state-quaternion-off-by-6e-6", 0.01, False, True, None, 1 + 6e-6)       # |q|^2 - 1 = 1.2e-5
    return out


def vio_prior_cases(n_generic=100, seed=821):
    """(name, prior state, state i, ok?) for prior_error / prior_linearize"""
    rng = np.random.default_rng(seed)
    out = []

    def case(name, rot, ok, qs=1.0, same=False):
        pr = _state(rng)
        pr[16:22] = rng.normal(0, 1e-3, 6)
        si = pr.copy()
        if not same:
            si[0:3] += rng.normal(0, 0.05, 3)
            si[3:6] += rng.normal(0, 0.05, 3)
            si[6:10] = synth_ba._R_to_quat(synth_ba.quat_to_R(pr[6:10]) @ synth_ba.so3_exp(np.asarray(rot, float)))
            si[10:22] += rng.normal(0, 1e-3, 12)
        si[6:10] *= qs
        out.append((name, pr, si, ok))
    case("identical", np.zeros(3), True, same=True)
    case("rotation-0.4895rad", 0.4895 * _unit(rng), True)
    case("rotation-0.4905rad", 0.4905 * _unit(rng), False)
    case("rotation-3rad", 3.0 * _unit(rng), False)
    case("rotation-1e-9rad", 1e-9 * _unit(rng), True)
    case("state-quaternion-unit-to-1e-7", 0.05 * _unit(rng), True, 1 + 1e-7)
    case("state-quaternion-off-by-6e-6", 0.05 * _unit(rng), False, 1 + 6e-6)
    for k in range(n_generic):
        th = 10.0 ** rng.uniform(-6, math.log10(0.48)) if k % 2 else rng.uniform(0.01, 0.48)
        case("generic-%d" % k, th * _unit(rng), True)
    return out


def vio_inc_cases(seed=831):
    """(name, state, dPVR, dBias, ok?) for ns_inc_unit: state_inc_cases and |dphi| 0.49, 0.51 and 3"""
    out = [(n, s, d, db, float(np.linalg.norm(d[6:9])) < 0.4999) for n, s, d, db in state_inc_cases()]
    assert not any(0.4999 <= float(np.linalg.norm(c[2][6:9])) <= 0.5001 for c in out)
    rng = np.random.default_rng(seed)
    for nn, th in (("0.49", 0.49), ("0.51", 0.51), ("3", 3.0)):
        for an, ax in AXES:
            s = np.concatenate([rng.uniform(-10, 10, 3), rng.normal(0, 1, 3), _quat(rng), rng.normal(0, 0.01, 3),
                                rng.normal(0, 0.1, 3), rng.normal(0, 1e-3, 3), rng.normal(0, 1e-2, 3)])
            out.append(("dphi-norm=%s/axis=%s" % (nn, an), s,
                        np.concatenate([rng.normal(0, 0.1, 3), rng.normal(0, 0.1, 3), th * np.array(ax)]),
                        rng.normal(0, 1e-3, 6), th < 0.5))
    return out


def vio_visual_cases(seed=841):
    """(camera table [n, 17]: fx fy cx cy bf Rcb tcb, slots): a slot is (name, camera, pose (p, q), observation (Xw, u, v,
    ur, inv_sigma2: float values), valid, robust, Huber width, the 27 sums before, index into visual_cases or None).
    Valid slots: every case of visual_cases through its frame's camera (a pinhole), the first 24 again without the
    robust kernel.  Slots that do not count: depth 0, negative depth and depth 1e-300."""
    names, cams, _ = cameras()
    body = names.index("pinhole-body")
    local = {0: 0, body: 1}
    tab = np.zeros((3, 17))
    for ci, k in local.items():
        c = cams[ci]
        assert int(c["model"]) == 0
        tab[k, 0:4] = [float(c["fx"]), float(c["fy"]), float(c["cx"]), float(c["cy"])]
        tab[k, 4] = camera_bf(c)
        tab[k, 5:14], tab[k, 14:17] = c["Rcb"], c["tcb"]
    tab[2] = tab[0]
    tab[2, 14:17] = [0.0, 0.0, 1e-300]
    assert (tab[0, 5:14] == np.eye(3).reshape(-1)).all() and not tab[0, 14:17].any()
    rng = np.random.default_rng(seed)
    slots = []
    vc = visual_cases()
    for k, (name, c0, rig, pose, ob, flags, delta) in enumerate(vc):
        slots.append((name, local[c0], pose, ob, 1, 1, delta, np.zeros(27), k))
    for k, (name, c0, rig, pose, ob, flags, delta) in enumerate(vc[:24]):
        slots.append((name + "/robust=false", local[c0], pose, ob, 1, 0, delta, np.zeros(27), k))
    ident = np.array([0.0, 0, 0, 1.0, 0, 0, 0])
    for name, cam, z in (("masked/depth=0", 0, 0.0), ("masked/depth=-2", 0, -2.0), ("masked/depth=1e-300", 2, 0.0)):
        for sn, ur in (("mono", -1.0), ("stereo", 300.0)):
            ob = np.array([0.125, -0.25, z, 320.0, 240.0, ur, 1.0])
            slots.append(("%s/%s" % (name, sn), cam, ident, ob, 0, 1, math.sqrt(7.815 if ur >= 0 else 5.991),
                          rng.normal(0, 100.0, 27), None))
    return tab, slots


def vio_huber_cases():
    """(name, e, delta, dsqr, robust): huber_cases through huber_flat, the named ones again with robust = false"""
    hc = huber_cases()
    return [(n, e, d, q, 1) for n, e, d, q in hc] + [(n + "/robust=false", e, d, q, 0) for n, e, d, q in hc[:18]]


def _spd(rng, n, cond):
    Q, _ = np.linalg.qr(rng.normal(0, 1, (n, n)))
    return (Q * np.logspace(0, math.log10(cond), n)) @ Q.T


def _vio_system(rng, n, cond=1e2, scale=None):
    """H (n x n) of the structure wave_solve_vio states: unknowns 9..14 meet only themselves and, for n = 30, 24 + t.
    Built from its Schur complement: a random SPD matrix on the other unknowns, to which the bias coupling's
    off_t^2 / d_t is added back."""
    keep = [i for i in range(n) if not 9 <= i < 15]
    H = np.zeros((n, n))
    S = _spd(rng, len(keep), cond)
    S = (S + S.T) / 2
    H[np.ix_(keep, keep)] = S
    for t in range(6):
        d = rng.uniform(1.0, 10.0)
        H[9 + t, 9 + t] = d
        if n == 30:
            off = -rng.uniform(0.2, 0.9) * d
            H[9 + t, 24 + t] = H[24 + t, 9 + t] = off
            H[24 + t, 24 + t] += off * off / d
    if scale is not None:
        H = H * np.outer(scale, scale)
    return H


def vio_solver_cases(seed=851):
    """(name, n, H, b, lambda, solvable?) for wave_solve_vio<9> (n = 15) and <24> (n = 30).  The first case stands
    again at the end (the first and the last workgroup)."""
    rng = np.random.default_rng(seed)
    out = []
    for n in (15, 30):
        b = lambda: rng.normal(0, 1, n)
        out.append(("n=%d/identity" % n, n, np.eye(n), b(), 0.0, True))
        out.append(("n=%d/diagonal" % n, n, np.diag(np.arange(1.0, n + 1)), b(), 0.0, True))
        for k in range(6):
            out.append(("n=%d/spd-cond-1e2-%d" % (n, k), n, _vio_system(rng, n), b(), 0.0, True))
        for k in range(4):
            sc = rng.permutation(np.logspace(-3, 4, n))
            H = _vio_system(rng, n, scale=sc)
            out.append(("n=%d/vio-scaled-%d" % (n, k), n, H, b() * sc, 0.0, True))
        H = _vio_system(rng, n)
        dg = np.diag(H)
        for ln, lam in (("0", 0.0), ("1e-8-mean-diagonal", 1e-8 * dg.mean()), ("smallest-diagonal", dg.min()),
                        ("10-largest-diagonal", 10 * dg.max())):
            out.append(("n=%d/lambda=%s" % (n, ln), n, H, b(), float(lam), True))
        # failing pivots: the eliminated ones, the first reduced one, one that turns negative under the updates, the last
        last = 8 if n == 15 else 29      # (n = 15: the reduced system is unknowns 0..8)
        for fn, (i, v) in (("eliminated-pivot-0-negative", (9, -1.0)), ("eliminated-pivot-5-nan", (14, float("nan"))),
                           ("eliminated-pivot-0-zero", (9, 0.0)), ("reduced-pivot-0-zero", (0, 0.0)),
                           ("reduced-pivot-0-nan", (0, float("nan"))), ("last-pivot-negative", (last, -1.0)),
                           ("last-pivot-nan", (last, float("nan")))):
            H = _vio_system(rng, n)
            H[i, i] = v
            out.append(("n=%d/%s" % (n, fn), n, H, b(), 0.0, False))
        H = np.eye(n)
        H[4, 5] = H[5, 4] = 2.0      # pivot 5 is 1 until pivot 4's update makes it 1 - 4
        out.append(("n=%d/middle-pivot-negative-after-updates" % n, n, H, b(), 0.0, False))
    # the bias coupling at the edge of definiteness: |off_t| within 1e-6 of sqrt(d_t d_(24+t)); rows 24 + t otherwise alone
    H = _vio_system(rng, 30)
    for t in range(6):
        H[24 + t, :] = 0
        H[:, 24 + t] = 0
        d, e = H[9 + t, 9 + t], rng.uniform(1.0, 10.0)
        H[24 + t, 24 + t] = e
        H[9 + t, 24 + t] = H[24 + t, 9 + t] = -math.sqrt(d * e) * (1 - 0.5e-6)
    out.append(("n=30/coupling-within-1e-6-of-singular", 30, H, rng.normal(0, 1, 30), 0.0, True))
    out.append((out[0][0] + "/again-in-the-last-workgroup",) + out[0][1:])
    return out
