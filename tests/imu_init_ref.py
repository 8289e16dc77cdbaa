"""IMUInitialization::TryInitVIO (reference src/Odom/IMUInitialization.cpp:1068-1480, the default path) restated in numpy
float64 -- the yardstick of vieo_imu_init -- and the same steps evaluated with 50 digits (mpmath) from the same inputs.

Only the new steps are new: the pre-integrations come from a pre-integrator the caller names (default: the CPU oracle's
restatement of IMUPreIntegratorBase::PreIntegration), in float64 for both evaluations.  One body of code serves both
arithmetics: it is written on numpy arrays with +, *, @ and a small namespace of scalar functions, float64 arrays for the
restatement, object arrays of mpf for the 50-digit evaluation.  The two differ in the least-squares solve alone: LAPACK's
SVD (numpy.linalg.svd) against the eigen-decomposition of A^T A with 50 digits (which loses twice the digits of the
condition number, 13 of 50 at cond 1e6 + guard).

float_rows=True casts to float32 wherever the reference holds a CV_32F (the rows, the solutions, RwI, the update's
matrices): what the reference itself would print, up to OpenCV's float SVD."""
import mpmath
import numpy as np

from vieo_slam_amd.imu_init import DEGENERATE_GRAVITY, FEW_EQUATIONS, FEW_KF, OK, REF_G

mpmath.mp.dps = 50


class _F64:
    name = "f64"
    sqrt, sin, cos, atan2 = staticmethod(np.sqrt), staticmethod(np.sin), staticmethod(np.cos), staticmethod(np.arctan2)

    @staticmethod
    def arr(x):
        return np.array(x, np.float64)

    @staticmethod
    def zeros(*shape):
        return np.zeros(shape)


class _MP:
    name = "mp"
    sqrt, sin, cos, atan2 = (staticmethod(mpmath.sqrt), staticmethod(mpmath.sin), staticmethod(mpmath.cos),
                             staticmethod(mpmath.atan2))

    @staticmethod
    def arr(x):
        a = np.asarray(x)
        out = np.empty(a.shape, object)
        for i, v in np.ndenumerate(a):
            out[i] = v if isinstance(v, mpmath.mpf) else mpmath.mpf(float(v))
        return out

    @staticmethod
    def zeros(*shape):
        return _MP.arr(np.zeros(shape))


def _eye(M):
    return M.arr(np.eye(3))


def _hat(M, w):
    z = w[0] * 0
    return np.array([[z, -w[2], w[1]], [w[2], z, -w[0]], [-w[1], w[0], z]], dtype=w.dtype)


def _norm(M, v):
    return M.sqrt(sum(x * x for x in v))


def so3_exp(M, w):
    th = _norm(M, w)
    O = _hat(M, w)
    if th < 1e-5:
        return _eye(M) + O + O @ O / 2
    return _eye(M) + O * (M.sin(th) / th) + O @ O * ((1 - M.cos(th)) / (th * th))


def R_to_q(M, R):
    """Eigen's Quaternion(Matrix3) + normalize, (w, x, y, z): what SO3ex(R) holds, also for an R that is a rotation only to
    float32 accuracy (the widened mTwc)"""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    q = [None] * 4
    if t > 0:
        t = M.sqrt(t + 1)
        q[0] = t / 2
        t = 1 / (2 * t)
        q[1], q[2], q[3] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = M.sqrt(R[i, i] - R[j, j] - R[k, k] + 1)
        q[1 + i] = t / 2
        t = 1 / (2 * t)
        q[0] = (R[k, j] - R[j, k]) * t
        q[1 + j], q[1 + k] = (R[j, i] + R[i, j]) * t, (R[k, i] + R[i, k]) * t
    q = np.array(q, dtype=R.dtype)
    return q / _norm(M, q)


def so3_log(M, R):
    """SO3ex::Log(R): through the unit quaternion of R"""
    q = R_to_q(M, R)
    n = _norm(M, q[1:])
    if n < 1e-12:
        return q[1:] * (2 / q[0])
    return q[1:] * (2 * M.atan2(n, q[0]) / n)


def so3_JrInv(M, w):
    th = _norm(M, w)
    O = _hat(M, w)
    if th < 1e-5:
        return _eye(M) + O / 2 + O @ O / 12
    return _eye(M) + O / 2 + O @ O * (1 / (th * th) - (1 + M.cos(th)) / (2 * th * M.sin(th)))


def _inv3(M, S):
    c = np.array([[S[1, 1] * S[2, 2] - S[1, 2] * S[2, 1], S[0, 2] * S[2, 1] - S[0, 1] * S[2, 2], S[0, 1] * S[1, 2] - S[0, 2] * S[1, 1]],
                  [S[1, 2] * S[2, 0] - S[1, 0] * S[2, 2], S[0, 0] * S[2, 2] - S[0, 2] * S[2, 0], S[0, 2] * S[1, 0] - S[0, 0] * S[1, 2]],
                  [S[1, 0] * S[2, 1] - S[1, 1] * S[2, 0], S[0, 1] * S[2, 0] - S[0, 0] * S[2, 1], S[0, 0] * S[1, 1] - S[0, 1] * S[1, 0]]],
                 dtype=S.dtype)
    det = S[0, 0] * c[0, 0] + S[0, 1] * c[1, 0] + S[0, 2] * c[2, 0]
    return c / det


def _solve3(M, H, b):
    """LDL^T of a symmetric positive definite 3 x 3; None when a pivot is not positive (g2o's solver fails)"""
    d0 = H[0, 0]
    if not d0 > 0:
        return None
    l10, l20 = H[0, 1] / d0, H[0, 2] / d0
    d1 = H[1, 1] - l10 * H[0, 1]
    if not d1 > 0:
        return None
    l21 = (H[1, 2] - l20 * H[0, 1]) / d1
    d2 = H[2, 2] - l20 * H[0, 2] - l21 * l21 * d1
    if not d2 > 0:
        return None
    y0 = b[0]
    y1 = b[1] - l10 * y0
    y2 = b[2] - l20 * y0 - l21 * y1
    z2 = y2 / d2
    z1 = y1 / d1 - l21 * z2
    z0 = y0 / d0 - l10 * z1 - l20 * z2
    return np.array([z0, z1, z2], dtype=H.dtype)


# ---------------------------------------------------------------- step 1
def gyro_edge(M, Rcb, Twc_i, Twc_j, P, prv):
    """EdgeGyrBias at bg = 0: (e, J, W)"""
    Rcb = M.arr(Rcb).reshape(3, 3)
    Rwbi, Rwbj = M.arr(Twc_i)[:, :3] @ Rcb, M.arr(Twc_j)[:, :3] @ Rcb
    dR, JgR = M.arr(P["Rij"]).reshape(3, 3), M.arr(P["JgR"]).reshape(3, 3)
    e = so3_log(M, dR.T @ Rwbi.T @ Rwbj)
    J = -(so3_JrInv(M, e) @ so3_exp(M, -e) @ JgR)
    W = _inv3(M, M.arr(np.asarray(prv).reshape(9, 9)[3:6, 3:6]))
    return e, J, W


def gyro_step(M, case, n, pre, prv):
    H, b, n_eq = M.zeros(3, 3), M.zeros(3), 0
    for i in range(1, n):
        if pre[i]["dt"] == 0:
            continue
        e, J, W = gyro_edge(M, case["Rcb"], case["Twc"][i - 1], case["Twc"][i], pre[i], prv[i])
        H, b, n_eq = H + J.T @ W @ J, b - J.T @ W @ e, n_eq + 1
    bg = _solve3(M, H, b) if n_eq >= 1 else None
    return (M.zeros(3) if bg is None else bg), n_eq


# ---------------------------------------------------------------- steps 3 and 4
def _triple(M, case, pre, i, f32):
    P2, P3 = pre[i + 1], pre[i + 2]
    dt12, dt23 = float(P2["dt"]), float(P3["dt"])
    if dt12 == 0 or dt23 == 0:
        return None
    c = (lambda x: M.arr(np.asarray(x, np.float32))) if f32 else M.arr
    T1, T2, T3 = (M.arr(case["Twc"][i + k]) for k in range(3))
    Rcb, pcb = c(np.asarray(case["Rcb"]).reshape(3, 3)), c(case["pcb"])
    dt12, dt23 = M.arr(dt12)[()], M.arr(dt23)[()]
    lam = (T2[:, 3] - T1[:, 3]) * dt23 + (T2[:, 3] - T3[:, 3]) * dt12
    beta = (dt12 * dt12 * dt23 + dt12 * dt23 * dt23) / 2
    R1, R2, R3 = T1[:, :3], T2[:, :3], T3[:, :3]
    gam = ((R1 - R2) @ pcb * dt23 + (R3 - R2) @ pcb * dt12 - R2 @ Rcb @ c(P3["pij"]) * dt12
           - R1 @ Rcb @ c(P2["vij"]) * (dt12 * dt23) + R1 @ Rcb @ c(P2["pij"]) * dt23)
    return lam, beta, gam, R1 @ Rcb, R2 @ Rcb, dt12, dt23, c


def rows_first(M, case, n, pre, f32=False):
    rows, n_eq = M.zeros(3 * (n - 2), 5), 0
    for i in range(n - 2):
        t = _triple(M, case, pre, i, f32)
        if t is None:
            continue
        lam, beta, gam = t[:3]
        rows[3 * i:3 * i + 3, 0], rows[3 * i:3 * i + 3, 4] = lam, gam
        for r in range(3):
            rows[3 * i + r, 1 + r] = beta
        n_eq += 1
    return rows, n_eq


def rows_second(M, case, n, pre, RwI, G, f32=False):
    rows = M.zeros(3 * (n - 2), 7)
    G = M.arr(G)[()]
    for i in range(n - 2):
        t = _triple(M, case, pre, i, f32)
        if t is None:
            continue
        lam, beta, gam, R1b, R2b, dt12, dt23, c = t
        P2, P3 = pre[i + 1], pre[i + 2]
        Jap23, Jav12, Jap12 = (c(np.asarray(x).reshape(3, 3)) for x in (P3["Jap"], P2["Jav"], P2["Jap"]))
        zeta = R2b @ Jap23 * dt12 + R1b @ Jav12 * (dt12 * dt23) - R1b @ Jap12 * dt23
        s = slice(3 * i, 3 * i + 3)
        rows[s, 0], rows[s, 1], rows[s, 2] = lam, -beta * (RwI[:, 1] * G), beta * (RwI[:, 0] * G)
        rows[s, 3:6], rows[s, 6] = zeta, gam - beta * (RwI[:, 2] * G)
    return rows, None


def _raise_small(w):
    return [x + 1e-10 if abs(x) < 1e-10 else x for x in w]


def solve_f64(rows):
    """x = V diag(1 / w) U^T B by LAPACK's SVD; |w| < 1e-10 raised by 1e-10; a direction whose singular value is below the
    rule's threshold takes U^T B from (A v_k) . B / w_k, 0 for w_k == 0 (there LAPACK's u_k is arbitrary)"""
    rows = np.asarray(rows, np.float64)
    A, B = rows[:, :-1], rows[:, -1]
    U, w, Vt = np.linalg.svd(A, full_matrices=False)
    utb = U.T @ B
    for k in range(len(w)):
        if w[k] < 1e-10:
            utb[k] = (A @ Vt[k]) @ B / w[k] if w[k] > 0 else 0.0
    wr = np.array(_raise_small(w))
    return Vt.T @ (utb / wr), np.sort(wr)[::-1]


def solve_mp(rows):
    """the same solution with 50 digits: A^T A = V diag(w^2) V^T, x = sum_k v_k (v_k . A^T B) / (w_k w'_k)"""
    rows = _MP.arr(rows)
    A, B = rows[:, :-1], rows[:, -1]
    nc = A.shape[1]
    E, Q = mpmath.eigsy(mpmath.matrix((A.T @ A).tolist()))
    AtB = A.T @ B
    x, w = _MP.zeros(nc), []
    for k in range(nc):
        wk = mpmath.sqrt(E[k]) if E[k] > 0 else mpmath.mpf(0)
        wr = _raise_small([wk])[0]
        w.append(wr)
        if wk > 0:
            v = np.array([Q[a, k] for a in range(nc)], dtype=object)
            x = x + v * ((v @ AtB) / (wk * wr))
    return x, np.array(sorted(w, reverse=True), dtype=object)


def solve_f32(rows):
    """the solve on CV_32F rows in float32 (numpy's float32 SVD stands in for OpenCV's)"""
    rows = np.asarray(rows, np.float64).astype(np.float32)
    A, B = rows[:, :-1], rows[:, -1]
    U, w, Vt = np.linalg.svd(A, full_matrices=False)
    w = np.array(_raise_small(w), np.float32)
    return (Vt.T @ ((U.T @ B) / w)).astype(np.float64), np.sort(w)[::-1].astype(np.float64)


def gravity_frame(M, gws):
    n = _norm(M, gws)
    if not n > 0:
        return None
    g = gws / n
    c = np.array([-g[1], g[0], g[0] * 0], dtype=gws.dtype)
    nc = _norm(M, c)
    if not nc > 0:
        return None
    return so3_exp(M, c / nc * M.atan2(nc, g[2]))


# ---------------------------------------------------------------- the whole call
def _intervals(case):
    t = np.asarray(case["t"], np.float64)
    return np.concatenate([t[:1], t[:-1]]), t


def default_preintegrate():
    from tests import oracle_lib
    return oracle_lib.load().imu_preintegrate


def restate(case, preintegrate=None, arith="f64", float_rows=False, shared=None):
    """TryInitVIO on one case (vieo_slam_amd.imu_init.try_init_vio's).  arith: "f64" (the restatement) or "mp" (50 digits).
    shared: the dict a previous call on the same case returned -- its pre-integrations are used again (the 50-digit
    evaluation shares the restatement's: they exist in float64 only).  Returns a dict: status, n_eq_gyro, n_eq, inited,
    bg, s_star, gw_star, w, RwI, s, dtheta, ba, w2, RwI_opt, gw, rows1, rows2, Tcw, nav_p, nav_q, nav_v, nav_set, preint,
    sigma_prv, points, pre (the three passes)."""
    M = _MP if arith == "mp" else _F64
    pre_fn = preintegrate or default_preintegrate()
    n_kf, n = len(case["Twc"]), case.get("n_kf_init", len(case["Twc"]))
    ti, tj = _intervals(case)
    G = case.get("ref_g", REF_G)
    zeros = np.zeros((n_kf, 3))
    R = dict(status=OK, n_eq_gyro=0, n_eq=0, inited=0, bg=M.zeros(3), nav_set=np.zeros(n_kf, np.int32), pre={})
    if shared is not None:
        R["pre"] = shared["pre"]
    if n < 4:
        R["status"] = FEW_KF
        return R
    if 0 not in R["pre"]:
        R["pre"][0] = ((case["preint"], np.asarray(case["preint_sigma_prv"]).reshape(-1, 81)) if case.get("preint") is not None
                       else pre_fn(case["noise"], case["samples"], ti, tj, zeros, zeros)[:2])
    pre0, prv0 = R["pre"][0]
    R["bg"], R["n_eq_gyro"] = gyro_step(M, case, n, pre0, np.asarray(prv0).reshape(-1, 81))
    if 1 not in R["pre"]:
        bgf = np.array([float(x) for x in R["bg"]])
        R["pre"][1] = pre_fn(case["noise"], case["samples"], ti, tj, np.tile(bgf, (n_kf, 1)), zeros)[:2]
    pre1 = R["pre"][1][0]
    rows1, R["n_eq"] = rows_first(M, case, n, pre1, float_rows)
    R["rows1"] = rows1
    if R["n_eq"] < 4:
        R["status"] = FEW_EQUATIONS
        return R
    solve = solve_f32 if float_rows else solve_mp if arith == "mp" else solve_f64
    x, R["w"] = solve(rows1)
    x = M.arr(x)
    R["s_star"], R["gw_star"] = x[0], x[1:4]
    RwI = gravity_frame(M, x[1:4])
    if RwI is None:
        R["status"] = DEGENERATE_GRAVITY
        return R
    if float_rows:
        RwI = M.arr(np.asarray(RwI, np.float32))
    R["RwI"] = RwI
    rows2, _ = rows_second(M, case, n, pre1, RwI, G, float_rows)
    R["rows2"] = rows2
    y, R["w2"] = solve(rows2)
    y = M.arr(y)
    R["s"], R["dtheta"], R["ba"] = y[0], y[1:3], y[3:6]
    R["RwI_opt"] = RwI @ so3_exp(M, np.array([y[1], y[2], y[0] * 0], dtype=y.dtype))
    R["gw"] = R["RwI_opt"][:, 2] * M.arr(G)[()]
    R["inited"] = int(bool(case.get("apply", 1)))
    if not R["inited"]:
        return R
    # ---- step 5
    if 3 not in R["pre"]:
        bgf, baf = np.array([float(v) for v in R["bg"]]), np.array([float(v) for v in R["ba"]])
        R["pre"][3] = pre_fn(case["noise"], case["samples"], ti, tj, np.tile(bgf, (n_kf, 1)), np.tile(baf, (n_kf, 1)))[:2]
    pre3, prv3 = R["pre"][3]
    R["preint"], R["sigma_prv"] = pre3, np.asarray(prv3).reshape(-1, 9, 9)
    s, gw = R["s"], R["gw"]
    Rcb, pcb = M.arr(np.asarray(case["Rcb"]).reshape(3, 3)), M.arr(case["pcb"])
    T = M.arr(case["Twc"])
    Tcw, P, Q, V = M.zeros(n_kf, 3, 4), M.zeros(n_kf, 3), M.zeros(n_kf, 4), M.zeros(n_kf, 3)

    def velocity(i, j):  # from the interval i -> j = i + 1
        dt, dp = M.arr(float(pre3[j]["dt"]))[()], M.arr(pre3[j]["pij"])
        return -(s * (T[i, :, 3] - T[j, :, 3]) + (T[i, :, :3] - T[j, :, :3]) @ pcb + gw * (dt * dt / 2)
                 + T[i, :, :3] @ Rcb @ dp) / dt

    for k in range(n_kf):
        Rwc, pwc = T[k, :, :3], T[k, :, 3]
        Tcw[k, :, :3], Tcw[k, :, 3] = Rwc.T, -(Rwc.T @ pwc) * s
        last = k == n_kf - 1
        j = k if last else k + 1
        if pre3[j]["dt"] == 0:
            continue  # the reference's `continue`
        P[k], Q[k] = s * pwc + Rwc @ pcb, R_to_q(M, Rwc @ Rcb)
        if not last:
            V[k] = velocity(k, k + 1)
        else:
            dt = M.arr(float(pre3[k]["dt"]))[()]
            V[k] = velocity(k - 1, k) + gw * dt + T[k - 1, :, :3] @ Rcb @ M.arr(pre3[k]["vij"])
        R["nav_set"][k] = 1
    R["Tcw"], R["nav_p"], R["nav_q"], R["nav_v"] = Tcw, P, Q, V
    pts = np.asarray(case.get("points", np.zeros(0, np.dtype([("pos", "<f4", 3), ("max_dist", "<f4"), ("min_dist", "<f4")]))))
    out = pts.copy()
    sf = np.float32(float(s))
    out["pos"], out["max_dist"], out["min_dist"] = pts["pos"] * sf, pts["max_dist"] * sf, pts["min_dist"] * sf
    R["points"] = out
    return R


def dist(a, b):
    """max |a - b| as a float (either side float64 or mpf)"""
    a, b = np.asarray(a, object).reshape(-1), np.asarray(b, object).reshape(-1)
    return float(max([abs(mpmath.mpf(x) - mpmath.mpf(y)) for x, y in zip(a, b)], default=0))


def tolerance(ref64, ref50):
    """16 x d_ref with a floor of 1e-13 relative: d_ref = the float64 restatement's distance from the 50-digit value of the
    same field; relative to the field's largest magnitude"""
    mag = float(max([abs(mpmath.mpf(x)) for x in np.asarray(ref50, object).reshape(-1)], default=0))
    d_ref = dist(ref64, ref50)
    return max(16 * d_ref, 1e-13 * mag), d_ref
