"""Named cases of the Sim3 algebra (vieo_slam_amd/csrc/sim3_device.h) for tests/test_sim3_algebra.py: plain float64
data, built without the code under test.  A Sim3 is [qx, qy, qz, qw, tx, ty, tz, s].

The switches sit at theta = eps and |sigma| = eps (exp), d = 1 - eps and |log s| = eps (log), trace = 0 and the ties of
the diagonal (matrix -> quaternion).  A case sits on a switch, one ulp to either side of it where its deciding value is
exact in a double (theta along a coordinate axis, sigma, hand-built traces), and 2 x 1e-12 (relative) to either side
where it is computed with roundings (theta along a generic axis, d): there 50 digits and a double could decide
differently any closer, and the test excuses nothing."""
import functools
import math
import os

import numpy as np

from tests import pose_graph_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "pose_graph_golden.npz")

SWITCH = 0.00001
BELOW, ABOVE = math.nextafter(SWITCH, 0.0), math.nextafter(SWITCH, 1.0)
OFF = 2e-12                      # 2 x EXCUSE_MARGIN: the nearest that a rounding of 1e-16 cannot carry into the margin
AXES = (("z", (0.0, 0.0, 1.0)), ("generic-a", (0.6, -0.48, 0.64)), ("generic-b", (-0.2672612419124244, 0.5345224838248488, 0.8017837257372732)))
NORM_OFFSETS = (0.0, 1e-16, -1e-16, 1e-12, -1e-12, 1e-8, -1e-8)


def _unit(q):
    q = np.asarray(q, np.float64)
    return q / np.linalg.norm(q)


def _axis_angle(axis, th):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([a * math.sin(th / 2), [math.cos(th / 2)]])


BASE_QUATS = (("identity", (0.0, 0.0, 0.0, 1.0)), ("generic", _unit((0.3, -0.5, 0.2, 0.79))),
              ("negative-w", _unit((0.1, 0.7, -0.4, -0.58))), ("half-turn-x", (1.0, 0.0, 0.0, 0.0)),
              ("near-half-turn", _axis_angle((0.2, -0.9, 0.4), math.pi - 1e-3)), ("small-angle", _axis_angle((0.5, 0.5, -0.7), 3e-6)))


@functools.lru_cache(maxsize=None)
def quat_cases():
    """(name, q): unit to the last bit, and with norm 1 +- {1e-16, 1e-12, 1e-8} as a product chain leaves them"""
    out = []
    for name, q in BASE_QUATS:
        for off in NORM_OFFSETS:
            out.append(("%s/norm=1%+.0e" % (name, off), np.asarray(q, np.float64) * (1.0 + off)))
    return out


@functools.lru_cache(maxsize=None)
def rot_cases():
    """(name, q, v) of s3_quat_rot"""
    vs = (("unit", (0.3, -2.0, 5.0)), ("1e4m", (1e4, -7e3, 2.5e3)), ("zero", (0.0, 0.0, 0.0)), ("axis", (0.0, 1.0, 0.0)))
    return [("%s/v=%s" % (n, vn), q, np.array(v)) for n, q in quat_cases() for vn, v in vs]


def _rotation(axis, th):
    return np.array(R.quat_to_mat([float(v) for v in _axis_angle(axis, th)]))


@functools.lru_cache(maxsize=None)
def mat_cases():
    """(name, R[9]) of s3_mat_to_quat: the four branches, the trace next to 0 on both sides, the ties.  The formula
    asks nothing of R, so the hand-built matrices are not rotations: their diagonals make the trace exact in a double
    ((0.5 - 0.25) exactly, then the third entry by Sterbenz), so 50 digits and a double see the same sign."""
    out = [("trace>0/identity", np.eye(3).reshape(-1)), ("trace>0/generic", _rotation((0.3, -0.5, 0.8), 0.7)),
           ("trace>0/100deg", _rotation((0.3, -0.5, 0.8), 1.75))]
    for i, ax in enumerate(((1.0, 0.05, -0.02), (0.03, 1.0, 0.04), (-0.05, 0.02, 1.0))):
        out.append(("i=%d/170deg" % i, _rotation(ax, 2.97)))
        out.append(("i=%d/pi-1e-3" % i, _rotation(ax, math.pi - 1e-3)))
    off = np.array([0.0, -0.31, 0.22, 0.31, 0.0, -0.4, -0.22, 0.4, 0.0])
    for tag, t8 in (("+1e-12", -0.25 + 1e-12), ("-1e-12", -0.25 - 1e-12), ("+1ulp", math.nextafter(-0.25, 0.0)),
                    ("-1ulp", math.nextafter(-0.25, -1.0)), ("=0", -0.25)):
        M = off.copy()
        M[0], M[4], M[8] = 0.5, -0.25, t8
        out.append(("trace%s" % tag, M))
    out.append(("trace=0/120deg-about-111", np.array([0.0, 0, 1, 1, 0, 0, 0, 1, 0])))
    for tag, dg in (("tie-R4=R0", (-0.2, -0.2, -0.7)), ("tie-R8=R4", (-0.7, -0.2, -0.2)), ("tie-R8=R0", (-0.2, -0.7, -0.2)),
                    ("tie-all", (-0.3, -0.3, -0.3)), ("half-turn-about-110", (0.0, 0.0, -1.0)), ("half-turn-about-011", (-1.0, 0.0, 0.0))):
        M = off.copy()
        M[0], M[4], M[8] = dg
        out.append((tag, M))
    return out


SCALES = (1e-3, 1.0, 1e3)
TRANSLATIONS = (("unit", (0.3, -1.2, 2.0)), ("1e4m", (1e4, -6e3, 8e3)), ("zero", (0.0, 0.0, 0.0)))


@functools.lru_cache(maxsize=None)
def sim3_cases():
    """(name, S[8]): every base quaternion at norm offsets 0, +1e-12, -1e-8, +1e-16, x scales x translations"""
    out = []
    for qn, q in BASE_QUATS:
        for off in (0.0, 1e-16, 1e-12, -1e-8):
            for s in SCALES:
                for tn, t in TRANSLATIONS:
                    out.append(("%s/norm=1%+.0e/s=%g/t=%s" % (qn, off, s, tn),
                                np.concatenate([np.asarray(q, np.float64) * (1.0 + off), t, [s]])))
    return out


@functools.lru_cache(maxsize=None)
def pair_cases():
    """(name, A[8], B[8]) of s3_mul: each case with a partner 7 places on, so scales and norms mix"""
    S = sim3_cases()
    return [("%s * %s" % (S[k][0], S[(k * 7 + 5) % len(S)][0]), S[k][1], S[(k * 7 + 5) % len(S)][1]) for k in range(0, len(S), 3)]


@functools.lru_cache(maxsize=None)
def map_cases():
    ps = (("unit", (0.3, -2.0, 5.0)), ("1e4m", (-1e4, 3e3, 50.0)))
    S = sim3_cases()
    return [("%s/p=%s" % (S[k][0], pn), S[k][1], np.array(p)) for k in range(0, len(S), 2) for pn, p in ps]


def thetas(axis_name):
    """the angles of exp: on the switch and one ulp off it where theta is exact (a coordinate axis), 2e-12 off it else"""
    lo, hi = (BELOW, ABOVE) if axis_name == "z" else (SWITCH * (1 - OFF), SWITCH * (1 + OFF))
    mid = (SWITCH,) if axis_name == "z" else ()
    return (0.0, lo) + mid + (hi, 1e-4, 0.5, 3.0, math.pi - 1e-3)


SIGMAS = (0.0, BELOW, -BELOW, SWITCH, -SWITCH, ABOVE, -ABOVE, 0.1, -0.3, 3.0)
UPSILONS = (("generic", (0.3, -1.2, 2.0)), ("zero", (0.0, 0.0, 0.0)), ("1e4", (1e4, -6e3, 8e3)))


@functools.lru_cache(maxsize=None)
def exp_cases():
    """(name, u[7]): theta x axis x sigma, upsilon generic everywhere and zero / 1e4 along the first generic axis"""
    out = []
    for an, ax in AXES:
        for th in thetas(an):
            for sg in SIGMAS:
                for un, up in UPSILONS:
                    if un != "generic" and an != "generic-a":
                        continue
                    w = [th * a for a in ax]
                    out.append(("theta=%.17g/axis=%s/sigma=%.17g/upsilon=%s" % (th, an, sg, un), np.array(w + list(up) + [sg])))
    return out


def _flat(S):
    return np.array(list(S[0]) + list(S[1]) + [S[2]])


def _tuple(a):
    return ([float(v) for v in a[0:4]], [float(v) for v in a[4:7]], float(a[7]))


@functools.lru_cache(maxsize=None)
def log_cases():
    """(name, S[8]) of the accuracy family: the float64 restatement's exp of every exp case (theta up to pi - 1e-3, every
    sigma; s = exp(1e-5) comes back as a sigma just under eps: exp took the general branch, log takes C = 1), quaternions
    about z with d on both sides of 1 - eps (d = 1 - 2 z^2 there, one rounding), and d = 1 from an identity of norm
    1 + 1e-12 (the diagonal of toRotationMatrix does not see w, so d cannot pass 1)."""
    lm = R.Libm(0)
    out = [("exp(" + n + ")", _flat(R.exp([float(v) for v in u], lm))) for n, u in exp_cases()]
    t, s = [0.3, -1.2, 2.0], 1.0
    for tag, th in (("theta=4.4e-3", 4.4e-3), ("theta=4.5e-3", 4.5e-3)):
        for an, ax in AXES:
            out.append(("%s/axis=%s" % (tag, an), np.concatenate([_axis_angle(ax, th), t, [s]])))
    for tag, dd in (("d=(1-eps)(1+2e-12)", (1 - SWITCH) * (1 + OFF)), ("d=(1-eps)(1-2e-12)", (1 - SWITCH) * (1 - OFF))):
        z = math.sqrt((1 - dd) / 2)
        for sg in (1.0, math.exp(0.1)):
            out.append(("%s/s=%g" % (tag, sg), np.array([0.0, 0.0, z, math.sqrt(1 - z * z), 0.3, -1.2, 2.0, sg])))
    out.append(("identity/norm=1+1e-12", np.array([0.0, 0.0, 0.0, 1.0 + 1e-12, 0.3, -1.2, 2.0, 1.0])))
    out.append(("identity/norm=1+1e-12/s=1.3", np.array([0.0, 0.0, 0.0, 1.0 + 1e-12, 0.3, -1.2, 2.0, 1.3])))
    return out


NEAR_PI = (("pi-1e-5", math.pi - 1e-5), ("pi-1e-7", math.pi - 1e-7), ("pi-1e-9", math.pi - 1e-9), ("pi", math.pi))


@functools.lru_cache(maxsize=None)
def log_near_pi_cases():
    """(name, S[8]) of the property family: the restatement's exp at theta = pi - 1e-5 ... pi, and unit quaternions with
    w = 0 (the rounding of their norm decides whether d passes -1)"""
    lm = R.Libm(0)
    out = []
    for tn, th in NEAR_PI:
        for an, ax in AXES:
            for sg in (0.0, 0.1):
                out.append(("exp(theta=%s/axis=%s/sigma=%g)" % (tn, an, sg),
                            _flat(R.exp([th * a for a in ax] + [0.3, -1.2, 2.0, sg], lm))))
    rng = np.random.default_rng(5)
    for k in range(8):
        v = rng.standard_normal(3)
        out.append(("w=0/random-%d" % k, np.concatenate([v / np.linalg.norm(v), [0.0, 0.3, -1.2, 2.0, 1.0]])))
    return out


@functools.lru_cache(maxsize=None)
def edge_cases():
    """(name, C[8], Si[8], Sj[8]) of s3_edge_error: every edge of the golden cases ring24 and scale16 at their first
    linearisation (C the measurement the restatement forms from the tables), and products that land on each branch of
    log: C = Sj = a generic similarity's pieces, Si chosen so that C Si Sj^-1 = exp(u)"""
    g = np.load(GOLDEN)
    out = []
    for case in ("ring24", "scale16"):
        Scw, prior = g[case + "/Scw"], g[case + "/Scw_prior"]
        ei, ej, kind = g[case + "/edge_i"], g[case + "/edge_j"], g[case + "/edge_kind"]
        meas = R.measurements([_tuple(a) for a in Scw], [_tuple(a) for a in prior], ei, ej, kind)
        for e in range(len(ei)):
            out.append(("%s/edge-%d" % (case, e), _flat(meas[e]), Scw[ei[e]].copy(), Scw[ej[e]].copy()))
    lm = R.Libm(0)
    C = _tuple(np.concatenate([_unit((0.2, 0.1, -0.4, 0.88)), [1.0, -2.0, 0.5, 1.1]]))
    Sj = _tuple(np.concatenate([_unit((-0.3, 0.6, 0.1, 0.73)), [0.4, 3.0, -1.0, 0.9]]))
    for th in (0.0, 3e-6, 1e-4, 4.4e-3, 4.5e-3, 0.5, 3.0):
        for sg in (0.0, 5e-6, -5e-6, 2e-5, 0.1, -0.3):
            u = [th * a for a in AXES[1][1]] + [0.3, -1.2, 2.0, sg]
            Si = R.mul(R.inverse(C), R.mul(R.exp(u, lm), Sj))
            out.append(("product/theta=%g/sigma=%g" % (th, sg), _flat(C), _flat(Si), _flat(Sj)))
    return out


# ---------------------------------------------------------------------------------------- OptimizeSim3's state functions
@functools.lru_cache(maxsize=None)
def raw_quat_cases():
    """(name, q) of s3o_quat_normalize: the quaternions above at lengths 1e-3, 1 and 1e3"""
    return [("%s/x%g" % (n, f), q * f) for n, q in quat_cases() for f in (1e-3, 1.0, 1e3)]


@functools.lru_cache(maxsize=None)
def from_sim3_cases():
    """(name, [R12[9], t12[3], s12]) of s3o_state_from_sim3: rotations of all four conversion branches"""
    rots = [c for c in mat_cases() if c[0].startswith(("trace>0", "i="))]
    return [("%s/t=%s/s=%g" % (n, tn, sc), np.concatenate([Rm, t, [sc]])) for n, Rm in rots for tn, t in TRANSLATIONS for sc in SCALES]


@functools.lru_cache(maxsize=None)
def state_cases():
    """(name, [p[3], q[4], s]) of s3o_state_to_sim3 and s3o_inc_small"""
    out = []
    for qn, q in BASE_QUATS:
        for off in (0.0, 1e-16, 1e-12, -1e-8):
            for tn, t in TRANSLATIONS[:2]:
                for sc in SCALES:
                    out.append(("%s/norm=1%+.0e/p=%s/s=%g" % (qn, off, tn, sc), np.concatenate([t, np.asarray(q, np.float64) * (1.0 + off), [sc]])))
    return out


DPHIS = (0.0, BELOW, SWITCH, ABOVE, 1.0, 3.0)


@functools.lru_cache(maxsize=None)
def inc_small_cases():
    """(name, state, [d[7], fix_scale]): |dphi| on the 1e-5 switch and one ulp off it along a coordinate axis (theta is
    exact there), 2e-12 off it along a generic axis, and 0, 1, 3; fix_scale on and off"""
    S = state_cases()
    out = []
    k = 0
    for an, ax in AXES[:2]:
        ths = DPHIS if an == "z" else (SWITCH * (1 - OFF), SWITCH * (1 + OFF), 1.0, 3.0)
        for th in ths:
            for dp in ((0.01, -0.02, 0.03), (0.0, 0.0, 0.0), (30.0, -20.0, 10.0)):
                for fix in (0.0, 1.0):
                    name, st = S[(7 * k) % len(S)]
                    k += 1
                    out.append(("dphi=%.17g/axis=%s/dp=%g/fix_scale=%d/%s" % (th, an, dp[0], fix, name), st,
                                np.array(list(dp) + [th * a for a in ax] + [0.05, fix])))
    return out


@functools.lru_cache(maxsize=None)
def huber_cases():
    """(name, [e2, delta, dsqr]): e2 = dsqr exactly, one ulp either side, 0 and 1e12; delta = (double)(float)sqrt(th2)"""
    out = []
    for th2 in (10.0, 7.815, 5.991):
        delta = float(np.float32(math.sqrt(th2)))
        dsqr = delta * delta
        for tag, e2 in (("=dsqr", dsqr), ("dsqr-1ulp", math.nextafter(dsqr, 0.0)), ("dsqr+1ulp", math.nextafter(dsqr, 1e9)),
                        ("0", 0.0), ("1e12", 1e12), ("0.3", 0.3), ("40", 40.0)):
            out.append(("th2=%g/e2%s" % (th2, tag), np.array([e2, delta, dsqr])))
    return out


def _pack(H, b, chi=0.0):
    return np.array([H[i][j] for i in range(7) for j in range(i, 7)] + list(b) + [chi])


@functools.lru_cache(maxsize=None)
def ldlt_synthetic_cases():
    """extras beside ldlt_golden_cases: (name, [acc[36], lambda, N], must_fail): J^T J of random 2 x 7 rows as s3o_add_edge
    accumulates them (40 edges, the columns scaled like a pose's: metres, radians, a scale), at lambda = 0, 1e-5 x the
    largest diagonal entry and 1e3; a system whose column 3 is zero (rank-deficient: the pivot is exactly 0) and a
    negated one, which must fail; for N = 6 row and column 6 of the accumulator hold a guard that must not reach x"""
    out = []
    for seed in range(4):
        rng = np.random.default_rng(40 + seed)
        J = rng.standard_normal((80, 7)) * np.array([300.0, 300.0, 300.0, 900.0, 900.0, 900.0, 2000.0]) * (0.1 if seed == 3 else 1.0)
        e = rng.standard_normal(80)
        H, b = J.T @ J, -(J.T @ e)
        for N in (6, 7):
            for tag, lam in (("0", 0.0), ("1e-5 max diagonal", 1e-5 * float(np.diag(H)[:N].max())), ("1e3", 1e3)):
                Hh, bb = H.copy(), b.copy()
                if N == 6:
                    Hh[6, :], Hh[:, 6], bb[6] = 1e300, 1e300, 1e300
                out.append(("seed-%d/N=%d/lambda=%s" % (seed, N, tag), np.concatenate([_pack(Hh, bb), [lam, N]]), False))
        Hz, bz = H.copy(), b.copy()
        Hz[3, :], Hz[:, 3], bz[3] = 0.0, 0.0, 0.0
        for N in (6, 7):
            out.append(("seed-%d/N=%d/column-3-zero" % (seed, N), np.concatenate([_pack(Hz, bz), [0.0, N]]), True))
            out.append(("seed-%d/N=%d/negated" % (seed, N), np.concatenate([_pack(-H, b), [0.0, N]]), True))
    return out


# ---------------------------------------------------------------------------------------- OptimizeSim3's edges
EDGE_CAMERAS = ("pinhole", "radtan0-k2", "kb8-0", "pinhole-body")


@functools.lru_cache(maxsize=None)
def edge_cameras():
    """[(name, camera of tests/loop_optimize_ref.py, image size)] from the table of tests/algebra_cases.py"""
    from tests import algebra_cases as AC
    names, cams, sizes = AC.cameras()
    out = []
    for n in EDGE_CAMERAS:
        c = cams[names.index(n)]
        model = int(c["model"])
        out.append((n, dict(model=model, num_k=int(c["num_k"]) if model == 1 else 0, fx=float(c["fx"]), fy=float(c["fy"]), cx=float(c["cx"]),
                            cy=float(c["cy"]), k=[float(a) for a in c["dist"]], Rcb=[float(a) for a in c["Rcb"]],
                            tcb=[float(a) for a in c["tcb"]]), sizes[names.index(n)]))
    return out


@functools.lru_cache(maxsize=None)
def s3o_edge_cases():
    """(name, [mode, camera, q[4], p[3], s, X[3], obs[2]]): both modes x four cameras x scales 0.5, 1, 2 x camera-frame
    points at depth 0.3, 5 and 50 m and on the rays of the image border's pixels (by the pinhole part of the model; half
    a pixel inside at the left and the top, where u = 0 itself would be a cancelled sum rounded to float) x
    an observation 0.3 px (inlier) or 5 px (outlier at th2 = 10) from the projection.  X is a float, as S3oCorr holds it."""
    from tests import loop_optimize_ref as LO
    lm = R.Libm(0)
    q = _unit((0.05, -0.08, 0.03, 0.99))
    Rwb = np.array(R.quat_to_mat([float(v) for v in q])).reshape(3, 3)
    p = np.array([0.4, -0.3, 0.2])
    out, k = [], 0
    for ci, (cn, cam, (w, h)) in enumerate(edge_cameras()):
        Rcb, tcb = np.array(cam["Rcb"]).reshape(3, 3), np.array(cam["tcb"])
        ray = lambda u, v: np.array([(u - cam["cx"]) / cam["fx"], (v - cam["cy"]) / cam["fy"], 1.0])
        pts = [("depth=0.3", ray(300.0, 200.0) * 0.3), ("depth=5", ray(500.0, 120.0) * 5.0), ("depth=50", ray(200.0, 400.0) * 50.0),
               ("border-left", ray(0.5, 0.6 * h) * 4.0), ("border-right-bottom", ray(w - 1.0, h - 1.0) * 7.0), ("border-top", ray(0.4 * w, 0.5) * 2.0)]
        for mode in (1, 2):
            for s in (0.5, 1.0, 2.0):
                for pn, Pc in pts:
                    if mode == 1:     # Pc = Rcb Rwb^T (s X - p) + tcb
                        X = (Rwb @ Rcb.T @ (Pc - tcb) + p) / s
                    else:             # Pc = (Rcb Rwb X + Rcb p + tcb) / s
                        X = Rwb.T @ Rcb.T @ (s * Pc - tcb - Rcb @ p)
                    X = X.astype(np.float32).astype(np.float64)
                    st = ([float(v) for v in p], [float(v) for v in q], s)
                    e0, _ = LO.edge(mode, cam, st, X[None], np.zeros((1, 2)), lm, want_J=False)
                    off = (0.3, -0.2) if k % 2 == 0 else (4.0, 3.0)
                    k += 1
                    obs = (-e0[0] + off).astype(np.float32).astype(np.float64)
                    out.append(("mode=%d/%s/s=%g/%s/%s" % (mode, cn, s, pn, "inlier" if off[0] < 1 else "outlier"),
                                np.concatenate([[mode, ci], q, p, [s], X, obs])))
    return out


def edge_cam_table():
    from tests import loop_optimize_ref as LO
    return np.array([LO.cam_flat(c) for _, c, _ in edge_cameras()])


HUBER_TH2 = 10.0


@functools.lru_cache(maxsize=None)
def add_edge_cases():
    """(name, [e[2], J[14], info, delta, dsqr]): e and J of every edge case as the restatement gives them, at the
    information of octave 0 and of octave 2 (1 / 1.2^4), Huber at th2 = 10; every other case is an outlier"""
    from tests import loop_optimize_ref as LO
    lm = R.Libm(0)
    cams = [c for _, c, _ in edge_cameras()]
    delta = float(np.float32(math.sqrt(HUBER_TH2)))
    out = []
    for k, (name, a) in enumerate(s3o_edge_cases()):
        st = ([float(v) for v in a[6:9]], [float(v) for v in a[2:6]], float(a[9]))
        e, J = LO.edge(int(a[0]), cams[int(a[1])], st, a[10:13][None], a[13:15][None], lm)
        info = 1.0 if k % 4 < 2 else float(np.float32(1.0 / 1.2 ** 4))
        out.append((name + "/info=%.3g" % info, np.concatenate([e[0], J[0].reshape(-1), [info, delta, delta * delta]])))
    return out


GOLDEN_LDLT = ("p10", "p10_fix", "p64", "p130_o5", "p13_o4_fix", "kb840", "radtan40", "radtan40_o5_fix")


def _lambdas(acc, N):
    diag = [acc[k] for k in (0, 7, 13, 18, 22, 25, 27)][:N]
    return (("0", 0.0), ("1e-5 max diagonal", 1e-5 * max(abs(d) for d in diag)), ("1e3", 1e3))


@functools.lru_cache(maxsize=None)
def ldlt_golden_cases():
    """(name, [acc[36], lambda, N], must_fail): the accumulators of the golden cases' first linearisation
    (tests/golden/loop_optimize_golden.npz through the restatement's edges, Huber and sums in edge order) at lambda = 0,
    1e-5 x the largest diagonal entry and 1e3, with the case's own N and the other one; and a rank-deficient system:
    every point on the optical axis of a pinhole at the identity, so nothing observes the rotation about that axis
    (column 5) -- lambda = 0 must fail.  For N = 6 row and column 6 hold a guard."""
    from tests import loop_optimize_ref as LO
    from tests.golden import make_loop_optimize_golden as gen
    lm = R.Libm(0)
    Z = np.load(os.path.join(HERE, "golden", "loop_optimize_golden.npz"))
    out = []

    def guard(acc, N):
        a = np.array(acc, np.float64)
        if N == 6:
            for k in (6, 12, 17, 21, 24, 26, 27, 34):
                a[k] = 1e300
        return a
    for name in GOLDEN_LDLT:
        kf1, kf2 = gen.unpack_kf(Z, name + "/kf1/"), gen.unpack_kf(Z, name + "/kf2/")
        prob, _, _ = LO.problem(kf1, kf2, Z[name + "/match_in"])
        fix = bool(Z[name + "/fix"])
        st = LO.state_from_sim3(Z[name + "/R12_in"], Z[name + "/t12_in"], float(Z[name + "/s12_in"]), lm)
        acc = LO._Run(prob, HUBER_TH2, fix, lm, "forward").linearize(st)
        for N in (6, 7):
            for tag, lam in _lambdas(acc, N):
                out.append(("%s/N=%d/lambda=%s" % (name, N, tag), np.concatenate([guard(acc, N), [lam, N]]), False))
    cam = dict(edge_cameras()[0][1])
    n = 24
    z = np.linspace(1.0, 9.0, n)
    X = np.stack([np.zeros(n), np.zeros(n), z], axis=1)
    rng = np.random.default_rng(3)
    obs = (np.array([cam["cx"], cam["cy"]]) + rng.standard_normal((n, 2)) * 0.5).astype(np.float32).astype(np.float64)
    prob = dict(X1=X, X2=X, cams=[cam], obs1=obs, obs2=obs[::-1].copy(), info1=np.ones(n), info2=np.ones(n), cam1=np.zeros(n, np.int64),
                cam2=np.zeros(n, np.int64))
    acc = LO._Run(prob, HUBER_TH2, False, lm, "forward").linearize(([0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0], 1.0))
    for N in (6, 7):
        out.append(("optical-axis/N=%d/lambda=0" % N, np.concatenate([guard(acc, N), [0.0, N]]), True))
        out.append(("optical-axis/N=%d/lambda=1e-5 max diagonal" % N, np.concatenate([guard(acc, N), [_lambdas(acc, N)[1][1], N]]), False))
        out.append(("negated-golden/N=%d" % N, np.concatenate([guard(-np.array(out[0][1][:36]), N), [0.0, N]]), True))
    return out


@functools.lru_cache(maxsize=None)
def ldlt_cases():
    return ldlt_golden_cases() + ldlt_synthetic_cases()
