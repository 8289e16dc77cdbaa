"""CPU restatement of Optimizer::OptimizeSim3 (reference src/Optimizer.cc:2689-2918) in numpy float64, written from the
reference's text: the correspondences, both modes of EdgeReproject<2, 6, 3, MODE> (src/Odom/g2otypes.h:321-549) with
their Jacobians AS WRITTEN THERE (MODE 2: scale = 1 / s, the state inverted, `tcw *= scale`, only the position block times
-Rbw, the scale column (J_s + Jproj tcw) (-scale^2)), the camera models' Project with its float rounding, Huber,
BaseMultiEdge's quadratic form with rho[1] only, g2o's Levenberg-Marquardt over the dense 7 x 7 (6 x 6) system by an
unpivoted LDL^T, NavState::IncSmall (p += R dp, R <- R Exp(dphi)), optimize(5) -> erase -> optimize(5 | 10) -> erase with
the `return 0` path and the stale read of the edge errors after a rejected last trial.

Every transcendental goes through the Libm object of tests/pose_graph_ref.py; `order` is the order in which the edges'
contributions to H, b and chi2 are summed: "forward" (edge order), "reversed", ("perm", seed), "lanes64" (64 strided
partial sums, then an adjacent-pair tree: what the kernel does).  The arithmetic of one edge is the same in all of them."""
import math

import numpy as np

from tests import pose_graph_ref as pg

DBL_MAX = float(np.finfo(np.float64).max)
_M64 = 0xFFFFFFFFFFFFFFFF


# ---------------------------------------------------------------------------------------------------------------------
# libm, scalar and elementwise
def _p1(lm, x, y):
    return lm._p(float(x), float(y))


def _pv(lm, x, y):
    """Libm._p on arrays"""
    v = int(getattr(lm, "variant", 0))
    if v == 0:
        return y
    bits = np.ascontiguousarray(x, np.float64).view(np.uint64)
    with np.errstate(over="ignore"):
        h = (bits ^ (bits >> np.uint64(29))) * np.uint64(0x9E3779B97F4A7C15) + np.uint64((v * 0xD1B54A32D192ED03) & _M64)
    k = (h >> np.uint64(61)) & np.uint64(3)
    ok = (y != 0) & np.isfinite(y)
    return np.where(ok & (k == 0), np.nextafter(y, np.inf), np.where(ok & (k == 1), np.nextafter(y, -np.inf), y))


def _vsqrt(lm, x):
    return _pv(lm, x, np.sqrt(x))


def _vatan2(lm, y, x):
    return _pv(lm, y, np.array([math.atan2(a, b) for a, b in zip(y, x)], np.float64))


def _dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


# ---------------------------------------------------------------------------------------------------------------------
# the cameras
def camera(rec, Tcr, pinhole=False):
    """CAMERA_DTYPE record + the 3 x 4 float GetTcr() -> what SetParams(cam) leaves in the edge (parameters widened)"""
    T = np.asarray(Tcr, np.float32).reshape(3, 4).astype(np.float64)
    model = 0 if pinhole else int(rec["model"])
    return dict(model=model, num_k=int(rec["num_k"]) if model == 1 else 0, fx=float(rec["fx"]), fy=float(rec["fy"]),
                cx=float(rec["cx"]), cy=float(rec["cy"]), k=[float(a) for a in rec["dist"]],
                Rcb=[float(a) for a in T[:, :3].reshape(-1)], tcb=[float(a) for a in T[:, 3]])


def cam_flat(c):
    """the 26 doubles tests/emul/sim3_opt_emul.cc reads"""
    return np.array([c["model"], c["num_k"], c["fx"], c["fy"], c["cx"], c["cy"]] + c["k"] + c["Rcb"] + c["tcb"], np.float64)


ROUND_UV = True  # Project returns Vec2data (float); the Jacobian test differentiates the unrounded function


def _f32(a):
    return a.astype(np.float32).astype(np.float64) if ROUND_UV else a


def project(c, P, lm, want_J=True):
    """camm::{Pinhole,Radtan,KB8}Camera::Project on P[n, 3]: (uv[n, 2] rounded to float, J[n, 6] or None)"""
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    fx, fy, cx, cy = c["fx"], c["fy"], c["cx"], c["cy"]
    J = None
    if c["model"] == 1:
        nk, kk = c["num_k"], c["k"]
        p0, p1 = kk[nk], kk[nk + 1]
        invz = 1 / z
        xn, yn = x * invz, y * invz
        x2, y2, xy = xn * xn, yn * yn, xn * yn
        r2 = x2 + y2
        fd, term = 1.0, 1.0
        for i in range(nk):
            term = term * r2
            fd = fd + kk[i] * term
        if want_J:
            fd2, coeff2, term = 0.0, 0.0, 1.0
            for i in range(2, nk):
                coeff2 += 2
                fd2 = fd2 + coeff2 * kk[i] * term
                term = term * r2
            # 3 * p[i] is an int times a float (Tdata) in the reference: a float product (camera_radtan.h:91, :95)
            p0x3, p1x3 = float(np.float32(3.0) * np.float32(p0)), float(np.float32(3.0) * np.float32(p1))
            du_dx = fx * invz * (fd + fd2 * x2 + 2 * (p0 * yn + p1x3 * xn))
            du_dy = fx * invz * (fd2 * xy + 2 * (p0 * xn + p1 * yn))
            du_dz = -(xn * du_dx + yn * du_dy)
            dv_dx = du_dy * fy / fx
            dv_dy = fy * invz * (fd + fd2 * y2 + 2 * (p1 * xn + p0x3 * yn))
            dv_dz = -(xn * dv_dx + yn * dv_dy)
            J = np.stack([du_dx, du_dy, du_dz, dv_dx, dv_dy, dv_dz], axis=1)
        xd = xn * fd + 2 * p0 * xy + p1 * (r2 + 2 * x2)
        yd = yn * fd + 2 * p1 * xy + p0 * (r2 + 2 * y2)
        return np.stack([_f32(fx * xd * 1.0 + cx), _f32(fy * yd * 1.0 + cy)], axis=1), J
    invz = 1.0 / z
    uv_p = np.stack([_f32(fx * x * invz + cx), _f32(fy * y * invz + cy)], axis=1)
    if want_J:
        invz2 = invz * invz
        zero = np.zeros_like(x)
        J = np.stack([fx * invz + zero, zero, -fx * x * invz2, zero, fy * invz + zero, -fy * y * invz2], axis=1)
    if c["model"] != 2:
        return uv_p, J
    kk = c["k"]
    x2, y2 = x * x, y * y
    r2 = x2 + y2
    r = _vsqrt(lm, r2)
    far = r > float(np.float32(1e-5))
    with np.errstate(all="ignore"):
        theta = _vatan2(lm, r, z)
        theta2 = theta * theta
        thetad = kk[3] * theta2
        thetad = thetad + kk[2]
        thetad = thetad * theta2
        thetad = thetad + kk[1]
        thetad = thetad * theta2
        thetad = thetad + kk[0]
        thetad = thetad * theta2
        thetad = thetad + 1
        thetad = thetad * theta
        mx, my = x * thetad / r, y * thetad / r
        uv_k = np.stack([_f32(fx * mx * 1.0 + cx), _f32(fy * my * 1.0 + cy)], axis=1)
        uv = np.where(far[:, None], uv_k, uv_p)
        if want_J:
            invr = 1.0 / r
            drx, dry = x * invr, y * invr
            tmp = 1.0 / (z * z + r2)
            dtx, dty = drx * z * tmp, dry * z * tmp
            dd = 9.0 * kk[3] * theta2
            dd = dd + 7.0 * kk[2]
            dd = dd * theta2
            dd = dd + 5.0 * kk[1]
            dd = dd * theta2
            dd = dd + 3.0 * kk[0]
            dd = dd * theta2
            dd = dd + 1.0
            invr2 = invr * invr
            tr = thetad * invr
            jxy = x * (dd * dty * r - y * tr) * invr2
            Jk = np.stack([fx * (x * r * dd * dtx + y2 * tr) * invr2, fx * jxy, -fx * x * dd * tmp, fy * jxy,
                           fy * (y * r * dd * dty + x2 * tr) * invr2, -fy * y * dd * tmp], axis=1)
            J = np.where(far[:, None], Jk, J)
    return uv, J


# ---------------------------------------------------------------------------------------------------------------------
# the state: (p[3], q[4] = x, y, z, w of mRwb, s)
def _sqrt1(lm, x):
    return _p1(lm, x, math.sqrt(x))


def _qnormalize(q, lm):
    n = _sqrt1(lm, q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return [q[0] / n, q[1] / n, q[2] / n, q[3] / n]


def state_from_sim3(R12, t12, s12, lm):
    q = _qnormalize(pg.mat_to_quat([float(a) for a in np.asarray(R12, np.float64).reshape(-1)], lm), lm)
    qwb = _qnormalize([-q[0], -q[1], -q[2], q[3]], lm)
    r = pg.quat_rot(qwb, [float(a) for a in t12])
    return ([-r[0], -r[1], -r[2]], qwb, float(s12))


def state_to_sim3(st, lm):
    p, qwb, s = st
    q = _qnormalize([-qwb[0], -qwb[1], -qwb[2], qwb[3]], lm)
    r = pg.quat_rot(q, p)
    return s, np.array(pg.quat_to_mat(q), np.float64).reshape(3, 3), np.array([-r[0], -r[1], -r[2]], np.float64)


def inc_small(st, d, fix_scale, lm):
    p, q, s = st
    r = pg.quat_rot(q, d[:3])
    p = [p[0] + r[0], p[1] + r[1], p[2] + r[2]]
    theta = _sqrt1(lm, d[3] * d[3] + d[4] * d[4] + d[5] * d[5])
    if theta < 1e-5:
        t2 = theta * theta
        imag, real = 0.5 - t2 / 48., 1.0 - t2 / 8.
    else:
        half = 0.5 * theta
        imag, real = lm.sin(half) / theta, lm.cos(half)
    e = _qnormalize([imag * d[3], imag * d[4], imag * d[5], real], lm)
    q = _qnormalize(pg.quat_mul(q, e), lm)
    return (p, q, s if fix_scale else s + d[6])


# ---------------------------------------------------------------------------------------------------------------------
# the edges
def edge(mode, c, st, X, obs, lm, want_J=True, parts=None):
    """EdgeReproject<2, 6, 3, mode> on X[n, 3], obs[n, 2] with one camera: (e[n, 2], J[n, 2, 7] or None); parts: a dict
    that receives Pc, Jproj, Rcw, Xw, tcw"""
    p, q, s = st
    Rwb = pg.quat_to_mat(q)
    Rcb, tcb = c["Rcb"], c["tcb"]
    scale = s
    if mode == 2:
        scale = 1. / scale
        twb = [-_dot3(Rwb[i], Rwb[3 + i], Rwb[6 + i], p[0], p[1], p[2]) for i in range(3)]
        Rcw = [_dot3(Rcb[3 * i], Rcb[3 * i + 1], Rcb[3 * i + 2], Rwb[j], Rwb[3 + j], Rwb[6 + j]) for i in range(3) for j in range(3)]
        tcw = [(-_dot3(Rcw[3 * i], Rcw[3 * i + 1], Rcw[3 * i + 2], twb[0], twb[1], twb[2]) + tcb[i]) * scale for i in range(3)]
    else:
        Rcw = [_dot3(Rcb[3 * i], Rcb[3 * i + 1], Rcb[3 * i + 2], Rwb[3 * j], Rwb[3 * j + 1], Rwb[3 * j + 2]) for i in range(3)
               for j in range(3)]
        tcw = [-_dot3(Rcw[3 * i], Rcw[3 * i + 1], Rcw[3 * i + 2], p[0], p[1], p[2]) + tcb[i] for i in range(3)]
    Xw = X * scale
    Pc = np.stack([_dot3(Rcw[3 * i], Rcw[3 * i + 1], Rcw[3 * i + 2], Xw[:, 0], Xw[:, 1], Xw[:, 2]) + tcw[i] for i in range(3)], axis=1)
    uv, Jp = project(c, Pc, lm, want_J)
    e = obs - uv
    if parts is not None:
        parts.update(Pc=Pc, Jproj=None if Jp is None else -Jp, Rcw=Rcw, Xw=Xw, tcw=tcw)
    if not want_J:
        return e, None
    Jp = -Jp
    J = np.zeros((len(X), 2, 7))
    for r in range(2):
        jp = [Jp[:, 3 * r], Jp[:, 3 * r + 1], Jp[:, 3 * r + 2]]
        A = [_dot3(jp[0], jp[1], jp[2], -Rcb[j], -Rcb[3 + j], -Rcb[6 + j]) for j in range(3)]
        J0 = [_dot3(jp[0], jp[1], jp[2], Rcw[j], Rcw[3 + j], Rcw[6 + j]) for j in range(3)]
        if mode == 2:
            M = [_dot3(jp[0], jp[1], jp[2], -Rcw[j], -Rcw[3 + j], -Rcw[6 + j]) for j in range(3)]
            v = [Xw[:, 0], Xw[:, 1], Xw[:, 2]]
            for j in range(3):
                J[:, r, j] = _dot3(A[0], A[1], A[2], -Rwb[j], -Rwb[3 + j], -Rwb[6 + j])
        else:
            M = [_dot3(jp[0], jp[1], jp[2], Rcb[j], Rcb[3 + j], Rcb[6 + j]) for j in range(3)]
            d0, d1, d2 = Xw[:, 0] - p[0], Xw[:, 1] - p[1], Xw[:, 2] - p[2]
            v = [_dot3(Rwb[j], Rwb[3 + j], Rwb[6 + j], d0, d1, d2) for j in range(3)]
            for j in range(3):
                J[:, r, j] = A[j]
        J[:, r, 3] = (M[0] * 0. + M[1] * v[2]) + M[2] * -v[1]
        J[:, r, 4] = (M[0] * -v[2] + M[1] * 0.) + M[2] * v[0]
        J[:, r, 5] = (M[0] * v[1] + M[1] * -v[0]) + M[2] * 0.
        js = _dot3(J0[0], J0[1], J0[2], X[:, 0], X[:, 1], X[:, 2])
        if mode == 2:
            js = (js + _dot3(jp[0], jp[1], jp[2], tcw[0], tcw[1], tcw[2])) * (-scale * scale)
        J[:, r, 6] = js
    return e, J


def huber(e2, delta, dsqr, lm):
    sq = _vsqrt(lm, e2)
    inl = e2 <= dsqr
    with np.errstate(all="ignore"):
        return np.where(inl, e2, 2 * sq * delta - dsqr), np.where(inl, 1.0, delta / sq)


def _both_edges(prob, st, lm, want_J):
    """per correspondence: e12, J12, e21, J21 (each over all n; erased ones are computed and ignored by the caller)"""
    n = len(prob["X1"])
    out = []
    for mode, X, obs, cam in ((1, prob["X2"], prob["obs1"], prob["cam1"]), (2, prob["X1"], prob["obs2"], prob["cam2"])):
        e, J = np.zeros((n, 2)), np.zeros((n, 2, 7))
        for ci in np.unique(cam):
            sel = np.flatnonzero(cam == ci)
            ee, JJ = edge(mode, prob["cams"][int(ci)], st, X[sel], obs[sel], lm, want_J)
            e[sel] = ee
            if want_J:
                J[sel] = JJ
        out += [e, J]
    return out


def _chi2(e, info):
    return e[:, 0] * (info * e[:, 0]) + e[:, 1] * (info * e[:, 1])


def ordered_sum(rows, k_of_row, order):
    """sum of rows[m, K] in the given order; k_of_row: the correspondence of every row (rows are in edge order)"""
    m = len(rows)
    if m == 0:
        return np.zeros(rows.shape[1])
    seq = lambda idx: np.cumsum(rows[idx], axis=0)[-1] if len(idx) else np.zeros(rows.shape[1])
    if order == "forward":
        return seq(np.arange(m))
    if order == "reversed":
        return seq(np.arange(m)[::-1])
    if isinstance(order, tuple) and order[0] == "perm":
        return seq(np.random.default_rng(order[1]).permutation(m))
    assert order == "lanes64"
    part = [seq(np.flatnonzero(k_of_row % 64 == lane)) for lane in range(64)]
    w = 1
    while w < 64:
        for lane in range(0, 64, 2 * w):
            part[lane] = part[lane] + part[lane + w]
        w *= 2
    return part[0]


def ldlt_solve(acc, lam, n):
    """(H + lam I) x = b on the leading n x n block of the packed upper triangle; None on a non-positive pivot"""
    L = [[0.0] * 7 for _ in range(7)]
    k = 0
    for i in range(7):
        for j in range(i, 7):
            L[j][i] = float(acc[k])
            k += 1
    D = [0.0] * n
    for j in range(n):
        d = L[j][j] + lam
        for q in range(j):
            d -= L[j][q] * L[j][q] * D[q]
        if not d > 0:
            return None
        D[j] = d
        for i in range(j + 1, n):
            a = L[i][j]
            for q in range(j):
                a -= L[i][q] * L[j][q] * D[q]
            L[i][j] = a / d
    y = [0.0] * n
    for i in range(n):
        a = float(acc[28 + i])
        for q in range(i):
            a -= L[i][q] * y[q]
        y[i] = a
    x = [0.0] * 7
    for i in range(n - 1, -1, -1):
        a = y[i] / D[i]
        for q in range(i + 1, n):
            a -= L[q][i] * x[q]
        x[i] = a
    return x


class _Run:
    def __init__(self, prob, th2, fix_scale, lm, order):
        self.prob, self.lm, self.order, self.dim = prob, lm, order, 6 if fix_scale else 7
        self.n = len(prob["X1"])
        th2 = np.float32(th2)
        self.th2 = float(th2)
        self.delta = float(np.sqrt(th2))  # const float deltaHuber = sqrt(th2)
        self.dsqr = self.delta * self.delta
        self.erased = np.zeros(self.n, np.int32)
        self.chi = np.zeros((self.n, 2))
        self.chi_check = np.zeros((2, self.n, 2))
        self.trace = []

    def _rows_k(self):
        act = np.flatnonzero(self.erased == 0)
        return act, np.repeat(act, 2)

    def linearize(self, st):
        e12, J12, e21, J21 = _both_edges(self.prob, st, self.lm, True)
        act, k_rows = self._rows_k()
        rows = np.zeros((2 * len(act), 36))
        for slot, (e, J, info) in enumerate(((e12, J12, self.prob["info1"]), (e21, J21, self.prob["info2"]))):
            e, J, info = e[act], J[act], info[act]
            c2 = _chi2(e, info)
            self.chi[act, slot] = c2
            r0, r1 = huber(c2, self.delta, self.dsqr, self.lm)
            w = r1 * info
            o0, o1 = -(info * e[:, 0]) * r1, -(info * e[:, 1]) * r1
            k = 0
            for i in range(7):
                a0, a1 = J[:, 0, i] * w, J[:, 1, i] * w
                for j in range(i, 7):
                    rows[slot::2, k] = a0 * J[:, 0, j] + a1 * J[:, 1, j]
                    k += 1
                rows[slot::2, 28 + i] = J[:, 0, i] * o0 + J[:, 1, i] * o1
            rows[slot::2, 35] = r0
        return ordered_sum(rows, k_rows, self.order)

    def errors(self, st):
        e12, _, e21, _ = _both_edges(self.prob, st, self.lm, False)
        act, k_rows = self._rows_k()
        rows = np.zeros((2 * len(act), 1))
        for slot, (e, info) in enumerate(((e12, self.prob["info1"]), (e21, self.prob["info2"]))):
            c2 = _chi2(e[act], info[act])
            self.chi[act, slot] = c2
            rows[slot::2, 0] = huber(c2, self.delta, self.dsqr, self.lm)[0]
        return float(ordered_sum(rows, k_rows, self.order)[0])

    def check(self, which):
        act = np.flatnonzero(self.erased == 0)
        self.chi_check[which, act] = self.chi[act]
        bad = act[(self.chi[act, 0] > self.th2) | (self.chi[act, 1] > self.th2)]
        self.erased[bad] = which + 1
        return len(bad)

    def optimize(self, st, iters):
        """SparseOptimizer::optimize(iters) + OptimizationAlgorithmLevenberg::solve; returns (st, iterations, trials)"""
        lm, dim = self.lm, self.dim
        it, n_it, n_tr, n_bad_it, lam, ni = 0, 0, 0, 0, -1.0, 2.0
        while True:
            acc = self.linearize(st)
            n_it += 1
            current = ini = float(acc[35])
            if it == 0:
                m, k = 0.0, 0
                for i in range(7):
                    if i < dim:
                        m = max(m, abs(float(acc[k])))
                    k += 7 - i
                lam, ni, n_bad_it = 1e-5 * m, 2.0, 0
            qmax = 0
            while True:
                backup = st
                x = ldlt_solve(acc, lam, dim)
                ok2 = x is not None
                if not ok2:
                    x = [0.0] * 7
                st = inc_small(st, x, dim == 6, lm)
                chi = self.errors(st)
                scale = 0.0
                for j in range(7):
                    scale += x[j] * (lam * x[j] + float(acc[28 + j]))
                temp = chi if ok2 else DBL_MAX
                rho = (current - temp) / ((scale if ok2 else 0.0) + 1e-3)
                accepted = rho > 0 and math.isfinite(temp)
                self.trace.append((current, temp, lam, 1.0 if accepted else 0.0))
                if accepted:
                    t = 2 * rho - 1
                    alpha = 1. - _p1(lm, t, math.pow(t, 3.0))
                    alpha = min(alpha, 2. / 3.)
                    lam *= max(1. / 3., alpha)
                    ni = 2.0
                    current = temp
                else:
                    lam *= ni
                    ni *= 2
                    st = backup
                qmax += 1
                n_tr += 1
                if not (rho < 0 and qmax < 10):
                    break
            terminate = qmax == 10 or rho == 0
            if not terminate:
                n_bad_it = n_bad_it + 1 if (ini - current) * 1e3 < ini else 0
                terminate = n_bad_it >= 3
            it += 1
            if terminate or it >= iters:
                return st, n_it, n_tr


def run(prob, st, th2=10.0, fix_scale=False, lm=None, order="forward"):
    """OptimizeSim3 after the edges are set.  prob: dict(X1, X2 [n, 3], obs1, obs2 [n, 2], info1, info2 [n], cam1, cam2 [n]
    (indices into cams), cams = [camera(...)]).  returns dict(st, n_inliers, n_bad, returned0, erased[n] (0 / 1 / 2),
    chi_check[2, n, 2], trace [(chi2 before, chi2 after, lambda, accepted)], iterations[2], trials[2])"""
    lm = pg.Libm(0) if lm is None else lm
    R = _Run(prob, th2, fix_scale, lm, order)
    st0 = st
    st, it0, tr0 = R.optimize(st, 5)
    n_bad = R.check(0)
    more = 10 if n_bad > 0 else 5
    out = dict(n_bad=n_bad, erased=R.erased, chi_check=R.chi_check, trace=R.trace, iterations=[it0, 0], trials=[tr0, 0])
    if R.n - n_bad < 10:
        out.update(st=st0, n_inliers=0, returned0=1)
        return out
    st, it1, tr1 = R.optimize(st, more)
    n_bad2 = R.check(1)
    out.update(st=st, n_inliers=R.n - n_bad - n_bad2, returned0=0, iterations=[it0, it1], trials=[tr0, tr1])
    return out


# ---------------------------------------------------------------------------------------------------------------------
# from key frames
def problem(kf1, kf2, match12):
    """the correspondences of a visit (Optimizer.cc:2757-2850) from two LoopKeyFrame: (prob, i1[n], i2[n])"""
    distort = bool(kf1.use_distort)
    if distort:
        cams = [camera(kf1.cams[c], kf1.Tcr[c]) for c in range(kf1.n_cams)] + [camera(kf2.cams[c], kf2.Tcr[c]) for c in range(kf2.n_cams)]
    else:
        cams = [camera(kf1.cams[0], kf1.Tcr[0], pinhole=True)]
    first2 = {}
    for k in range(len(kf2.keys) - 1, -1, -1):
        if kf2.mp_id[k] >= 0:
            first2[int(kf2.mp_id[k])] = k
    i1 = [i for i in range(len(kf1.keys)) if match12[i] >= 0 and kf2.mp_id[match12[i]] >= 0 and kf1.mp_id[i] >= 0]
    m = [int(match12[i]) for i in i1]
    i2 = [first2[int(kf2.mp_id[k])] for k in m]

    def cam_points(kf, idx):
        R, t, X = kf.Rcw.astype(np.float32).reshape(3, 3), kf.tcw.astype(np.float32), kf.points["Xw"][idx].astype(np.float32).reshape(-1, 3)
        return np.stack([((R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1]) + R[r, 2] * X[:, 2]) + t[r] for r in range(3)], axis=1).astype(np.float64)
    i1a, i2a, ma = np.array(i1, np.int64), np.array(i2, np.int64), np.array(m, np.int64)
    prob = dict(X1=cam_points(kf1, i1a), X2=cam_points(kf2, ma), cams=cams,
                obs1=np.stack([kf1.keys["x"][i1a], kf1.keys["y"][i1a]], axis=1).astype(np.float64).reshape(-1, 2),
                obs2=np.stack([kf2.keys["x"][i2a], kf2.keys["y"][i2a]], axis=1).astype(np.float64).reshape(-1, 2),
                info1=kf1.inv_level_sigma2[kf1.keys["octave"][i1a]].astype(np.float64),
                info2=kf2.inv_level_sigma2[kf2.keys["octave"][i2a]].astype(np.float64),
                cam1=kf1.cam_of_key[i1a].astype(np.int64) if distort else np.zeros(len(i1), np.int64),
                cam2=(kf1.n_cams + kf2.cam_of_key[i2a]).astype(np.int64) if distort else np.zeros(len(i1), np.int64))
    return prob, i1a, i2a


def optimize_sim3(kf1, kf2, s12, R12, t12, match12, th2=10.0, fix_scale=False, lm=None, order="forward"):
    """int Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale): (match12 after the call, (s12, R12,
    t12) after the call, nInliers, detail).  A visit without a correspondence: 0, nothing changes."""
    lm = pg.Libm(0) if lm is None else lm
    match12 = np.array(match12, np.int32)
    S_in = (float(s12), np.array(R12, np.float64).reshape(3, 3), np.array(t12, np.float64))
    prob, i1, i2 = problem(kf1, kf2, match12)
    if len(i1) == 0:
        return match12, S_in, 0, None
    d = run(prob, state_from_sim3(S_in[1], S_in[2], S_in[0], lm), th2, fix_scale, lm, order)
    match12[i1[d["erased"] > 0]] = -1
    d["i1"], d["i2"], d["n_correspondences"] = i1, i2, len(i1)
    return match12, (S_in if d["returned0"] else state_to_sim3(d["st"], lm)), d["n_inliers"], d
