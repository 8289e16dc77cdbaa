"""The lane functions of vieo_imu_init (vieo_slam_amd/csrc/imu_init_device.h) on the host with 1 and 64 lanes
(tests/emul/imu_init_emul.cc): the Jacobi SVD solve against 50-digit values on planted matrices, the gyro edge against
central differences and the restatement, steps 1-4 and the closed forms of step 5 against the restatement, the degenerate
gravity guard.

Tolerance (tests/imu_init_ref.tolerance): 16 x d_ref with a floor of 1e-13 relative, d_ref = the distance of the float64
restatement (LAPACK's SVD) from the 50-digit solution of the same problem.  The factor covers another summation order
(wave tree against sequential) and Jacobi against bidiagonalisation, not a wrong rotation."""
import ctypes
import functools
import os
import subprocess

import mpmath
import numpy as np
import pytest

from tests import imu_init_ref as ref
from vieo_slam_amd import imu_init as ii

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p


@functools.lru_cache(maxsize=None)
def emul():
    out = os.path.join(ROOT, "tests", "emul", "libimu_init_emul.so")
    deps = [os.path.join(ROOT, "tests", "emul", "imu_init_emul.cc"),
            os.path.join(ROOT, "vieo_slam_amd", "csrc", "imu_init_device.h"), os.path.join(ROOT, "include", "vieo_hot.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-o", out, deps[0], "-lm"])
    L = ctypes.CDLL(out)
    L.emul_ii_gyro_edge.argtypes = [P] * 8
    L.emul_ii_jacobi.argtypes = [ctypes.c_int] * 3 + [P] * 3
    L.emul_ii_gravity_frame.argtypes = [P, P]
    L.emul_ii_steps.argtypes = [ctypes.c_int, ctypes.c_int] + [P] * 6 + [ctypes.c_double] + [P] * 3
    L.emul_ii_apply_kf.argtypes = [P, P, ctypes.c_int, P, P, ctypes.c_double] + [P] * 6
    assert L.emul_ii_max_sweeps() == ii.MAX_SWEEPS
    return L


def jacobi(n_lanes, rows):
    rows = np.ascontiguousarray(rows, np.float64)
    m, nc = rows.shape[0], rows.shape[1] - 1
    x, w = np.zeros(nc), np.zeros(nc)
    sweeps = emul().emul_ii_jacobi(n_lanes, m, nc, rows.ctypes.data, x.ctypes.data, w.ctypes.data)
    return x, w, sweeps


def _planted(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("random"):
        m, nc = (int(v) for v in name.split("_")[1:])
        return rng.normal(size=(m, nc + 1))
    if name == "cond_1e6":  # U diag(1 .. 1e-6) V^T
        U, _ = np.linalg.qr(rng.normal(size=(30, 6)))
        V, _ = np.linalg.qr(rng.normal(size=(6, 6)))
        A = U @ np.diag(np.logspace(0, -6, 6)) @ V.T
        return np.hstack([A, rng.normal(size=(30, 1))])
    if name == "zero_column":  # the +1e-10 rule
        R = rng.normal(size=(12, 7))
        R[:, 2] = 0
        return R
    if name == "zero_row_triples":  # skipped equations
        R = rng.normal(size=(21, 7))
        R[3:6] = 0
        R[15:18] = 0
        return R
    raise KeyError(name)


# 12 x 4 and 12 x 6: the smallest that pass the gate; 189 / 192 / 195 x 6: 63, 64 and 65 triples
PLANTED = ["random_12_4", "random_12_6", "random_189_6", "random_192_6", "random_195_6", "cond_1e6", "zero_column",
           "zero_row_triples"]


@pytest.mark.parametrize("name", PLANTED)
def test_jacobi_solve_against_50_digits(name):
    rows = _planted(name)
    x50, w50 = ref.solve_mp(rows)
    x64, w64 = ref.solve_f64(rows)
    tol_x, d_x = ref.tolerance(x64, x50)
    tol_w, d_w = ref.tolerance(w64, w50)
    x1, w1, s1 = jacobi(1, rows)
    xw, ww, sw = jacobi(64, rows)
    xw2, ww2, sw2 = jacobi(64, rows)
    print("%s: d_ref x %.2e w %.2e | 1 lane x %.2e w %.2e sweeps %d | 64 lanes x %.2e w %.2e sweeps %d | cond %.3g"
          % (name, d_x, d_w, ref.dist(x1, x50), ref.dist(w1, w50), s1, ref.dist(xw, x50), ref.dist(ww, w50), sw,
             float(w50[0] / w50[-1])))
    assert 1 <= s1 < ii.MAX_SWEEPS and 1 <= sw < ii.MAX_SWEEPS  # ended by a sweep without a rotation
    assert ref.dist(x1, x50) <= tol_x and ref.dist(w1, w50) <= tol_w
    assert ref.dist(xw, x50) <= tol_x and ref.dist(ww, w50) <= tol_w
    assert ref.dist(xw, x1) <= tol_x and ref.dist(ww, w1) <= tol_w  # 64 lanes against 1 lane
    assert xw.tobytes() == xw2.tobytes() and ww.tobytes() == ww2.tobytes() and sw == sw2  # run to run
    assert all(ww[k] >= ww[k + 1] for k in range(len(ww) - 1))
    if name == "zero_column":
        assert ww[-1] == 1e-10 and w1[-1] == 1e-10  # 0 raised by 1e-10
        assert xw[2] == 0 and x1[2] == 0            # a zero column has (U^T B)_k = 0


@functools.lru_cache(maxsize=None)
def _case(seed, n, step, s_true, empty=()):
    c = ii.make_init_case(seed, n, step, s_true, empty=empty)
    R = ref.restate(c)
    return c, R, ref.restate(c, arith="mp", shared=R)


def _emul_edge(Rcb, Ti, Tj, rec, prv):
    e, J, W = np.zeros(3), np.zeros((3, 3)), np.zeros((3, 3))
    emul().emul_ii_gyro_edge(Rcb.ctypes.data, Ti.ctypes.data, Tj.ctypes.data, rec.ctypes.data, prv.ctypes.data,
                             e.ctypes.data, J.ctypes.data, W.ctypes.data)
    return e, J, W


def _central_differences(Rcb, Ti, Tj, P):
    """d e / d bg at 0 of e(bg) = Log((dRij Exp(JgR bg))^T Rwbi^T Rwbj), with 50 digits and h = 1e-20"""
    M = ref._MP
    Rwbi, Rwbj = M.arr(Ti)[:, :3] @ M.arr(Rcb), M.arr(Tj)[:, :3] @ M.arr(Rcb)
    dR, JgR = M.arr(P["Rij"]).reshape(3, 3), M.arr(P["JgR"]).reshape(3, 3)
    h, J = mpmath.mpf(10) ** -20, M.zeros(3, 3)
    for k in range(3):
        d = M.zeros(3)
        d[k] = h
        ep = ref.so3_log(M, (dR @ ref.so3_exp(M, JgR @ d)).T @ Rwbi.T @ Rwbj)
        em = ref.so3_log(M, (dR @ ref.so3_exp(M, JgR @ -d)).T @ Rwbi.T @ Rwbj)
        J[:, k] = (ep - em) / (2 * h)
    return J


def _exact_rotation(T):
    T = np.array(T, np.float64)
    T[:, :3] = ref.so3_exp(ref._F64, ref.so3_log(ref._F64, T[:, :3]))  # orthonormal to float64 rounding
    return T


def test_gyro_edge_against_central_differences_and_the_restatement():
    c, R, _ = _case(3, 6, 10, 1.0)
    pre, prv = R["pre"][0]
    prv = np.ascontiguousarray(prv).reshape(-1, 81)
    Rcb = np.ascontiguousarray(c["Rcb"], np.float64)
    for i in range(1, 6):
        Ti, Tj = np.ascontiguousarray(c["Twc"][i - 1]), np.ascontiguousarray(c["Twc"][i])
        rec = np.ascontiguousarray(pre[i:i + 1])
        e, J, W = _emul_edge(Rcb, Ti, Tj, rec, prv[i])
        e64, J64, W64 = ref.gyro_edge(ref._F64, Rcb, Ti, Tj, pre[i], prv[i])
        e50, J50, W50 = ref.gyro_edge(ref._MP, Rcb, Ti, Tj, pre[i], prv[i])
        for got, r64, r50 in ((e, e64, e50), (J, J64, J50), (W, W64, W50)):
            tol, _ = ref.tolerance(r64, r50)
            assert ref.dist(got, r50) <= tol
        # The analytic Jacobian is the derivative for ROTATIONS; through the normalised quaternion of a matrix that is not
        # one, the two differ in proportion to the orthonormality defect max |R^T R - I| of the inputs (a few entries of it
        # per product: 8 x).  The widened mTwc carries float32 rounding (defect ~ 2^-24); the same poses made orthonormal
        # to float64 rounding leave the defect of dRij and Rcb.
        jmax = float(np.abs(J).max())
        for Ta, Tb in ((Ti, Tj), (_exact_rotation(Ti), _exact_rotation(Tj))):
            defect = max(_defect(Ta[:, :3]), _defect(Tb[:, :3]), _defect(Rcb.reshape(3, 3)), _defect(pre[i]["Rij"].reshape(3, 3)))
            e, J, W = _emul_edge(Rcb, Ta, Tb, rec, prv[i])
            d = ref.dist(J, _central_differences(Rcb, Ta, Tb, pre[i]))
            print("key frame %d: defect %.2e, J against central differences %.2e" % (i, defect, d))
            assert d <= 8 * defect * jmax


def _defect(R):
    R = ref._MP.arr(R)
    return ref.dist(R.T @ R, np.eye(3))


def _steps(n_lanes, c, R):
    n = c.get("n_kf_init", len(c["Twc"]))
    Twc = np.ascontiguousarray(c["Twc"], np.float64)
    pre0, prv0 = R["pre"][0]
    pre0, prv0 = np.ascontiguousarray(pre0), np.ascontiguousarray(prv0, np.float64)
    pre1 = np.ascontiguousarray(R["pre"][1][0])
    Rcb, pcb = np.ascontiguousarray(c["Rcb"], np.float64), np.ascontiguousarray(c["pcb"], np.float64)
    out = np.zeros(1, ii.IMU_INIT_RESULT_DTYPE)
    emul().emul_ii_steps(n_lanes, n, Twc.ctypes.data, pre0.ctypes.data, prv0.ctypes.data, pre1.ctypes.data, Rcb.ctypes.data,
                         pcb.ctypes.data, c.get("ref_g", ii.REF_G), out.ctypes.data, None, None)
    return out[0]


FIELDS = ("bg", "s_star", "gw_star", "w", "RwI", "s", "dtheta", "ba", "w2", "RwI_opt", "gw")


@pytest.mark.parametrize("seed,n,step,s_true,empty", [(3, 6, 10, 1.0, ()), (3, 21, 10, 1.0, ()), (5, 31, 10, 1.7, ()),
                                                      (7, 12, 5, 1.0, ()), (3, 67, 2, 1.0, ()), (3, 12, 10, 1.0, (5,))])
def test_steps_1_to_4_against_the_restatement(seed, n, step, s_true, empty):
    c, R, R50 = _case(seed, n, step, s_true, empty)
    r1, rw, rw2 = _steps(1, c, R), _steps(64, c, R), _steps(64, c, R)
    assert rw.tobytes() == rw2.tobytes()
    for r in (r1, rw):
        assert (r["status"], r["n_eq_gyro"], r["n_eq"]) == (R["status"], R["n_eq_gyro"], R["n_eq"]) == (
            ii.OK, n - 1 - len(empty), n - 2 - 2 * len(empty))
        for f in FIELDS:
            tol, d_ref = ref.tolerance(R[f], R50[f])
            d = ref.dist(r[f], R50[f])
            print("%s: d_ref %.2e tol %.2e emulation %.2e" % (f, d_ref, tol, d))
            assert d <= tol, f


def test_gravity_along_gI_is_degenerate():
    RwI = np.zeros(9)
    for g in ([0, 0, 9.8], [0, 0, -9.8], [0, 0, 0]):
        g = np.array(g, np.float64)
        assert emul().emul_ii_gravity_frame(g.ctypes.data, RwI.ctypes.data) == 0
    g = np.array([0.1, -0.2, 9.8])
    assert emul().emul_ii_gravity_frame(g.ctypes.data, RwI.ctypes.data) == 1
    assert ref.dist(RwI.reshape(3, 3) @ [0, 0, 1], g / np.linalg.norm(g)) < 1e-15  # RwI gI = gwn
    c = ii.make_static_case(6)
    R = ref.restate(c)
    assert R["status"] == ii.DEGENERATE_GRAVITY
    for lanes in (1, 64):
        r = _steps(lanes, c, R)
        assert r["status"] == ii.DEGENERATE_GRAVITY and r["n_eq"] == 4 and r["gw_star"][0] == 0 and r["gw_star"][1] == 0
        assert abs(r["gw_star"][2] + 9.8) < 1e-12


@pytest.mark.parametrize("seed,n,step,s_true,empty", [(3, 6, 10, 1.0, ()), (5, 31, 10, 1.7, ()), (3, 12, 10, 1.0, (5,))])
def test_step_5_closed_forms_against_the_restatement(seed, n, step, s_true, empty):
    """scaled Tcw, pwb, Rwb and the velocity (the inner key frames' formula and the last one's) from the restatement's own
    s, gw and re-integrated intervals"""
    c, R, R50 = _case(seed, n, step, s_true, empty)
    Rcb, pcb = np.ascontiguousarray(c["Rcb"], np.float64), np.ascontiguousarray(c["pcb"], np.float64)
    gw, pre3 = np.array([float(x) for x in R["gw"]]), np.ascontiguousarray(R["preint"])
    Tcw, p, q, v = np.zeros((n, 3, 4)), np.zeros((n, 3)), np.zeros((n, 4)), np.zeros((n, 3))
    on = R["nav_set"] == 1
    assert list(np.flatnonzero(~on)) == [k - 1 for k in empty]
    for k in np.flatnonzero(on):
        last = k == n - 1
        T, To = np.ascontiguousarray(c["Twc"][k]), np.ascontiguousarray(c["Twc"][k - 1 if last else k + 1])
        rec = pre3[k:k + 1] if last else pre3[k + 1:k + 2]
        emul().emul_ii_apply_kf(T.ctypes.data, To.ctypes.data, int(last), Rcb.ctypes.data, pcb.ctypes.data, float(R["s"]),
                                gw.ctypes.data, np.ascontiguousarray(rec).ctypes.data, Tcw[k].ctypes.data, p[k].ctypes.data,
                                q[k].ctypes.data, v[k].ctypes.data)
    for got, f in ((Tcw[on], "Tcw"), (p[on], "nav_p"), (q[on], "nav_q"), (v[on], "nav_v")):
        tol, d_ref = ref.tolerance(R[f][on], R50[f][on])
        d = ref.dist(got, R50[f][on])
        print("%s: d_ref %.2e tol %.2e emulation %.2e" % (f, d_ref, tol, d))
        assert d <= tol, f
