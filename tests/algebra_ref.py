"""The lane functions of ba_device.h / imu_device.h / cam_project.h / cam_unproject.h restated in mpmath at 50 digits.
Test infrastructure only.

Every function exists in up to two statements:

  *_aw   "as written": the reference's formula with its branch and its float roundings, evaluated without FP64 error.
         The constants are the doubles (or floats) the reference's compiler sees: 1e-5, M_PI, 1e-5f, 1e-8f.
  *_ex   "exact": the mathematical definition (exp / log of SO(3), the right Jacobian as its power series, the
         derivative of a projection by central differences at h = 1e-15, where truncation is about 1e-30).

Written from the reference's text (file and lines at each function); nothing here is derived from the device code or
from oracle/.  Inputs are Python floats (every double is an exact mpf); outputs are lists of mpf.
"""
import math

import mpmath
import numpy as np
from mpmath import mp, mpf

mp.dps = 50

SMALL_EPS = mpf(1e-5)            # so3_extra.h:233, a double
M_PI = mpf(math.pi)              # the double the reference's M_PI is
PRECISION_R = mpf(float(np.float32(1e-5)))   # camera_kb8.h:61, const float precision_r_ = 1e-5
PRECISION = mpf(float(np.float32(1e-8)))     # camera_base.h:123, float precision_ = 1e-8
MAX_ITER = 10                    # camera_base.h:122, num_max_iteration_
H_FD = mpf(10) ** -15


def V(x):
    return [mpf(float(t)) for t in x]


def f32(x):
    """x rounded to the nearest float (ties to even), as an mpf; the normal range only"""
    x = mpf(x)
    if x == 0:
        return x
    return mpmath.mpf(mpmath.libmp.mpf_pos(x._mpf_, 24, "n"))


def f32_margin(x):
    """relative distance of x from the nearest point at which its float rounding changes"""
    x = mpf(x)
    if x == 0:
        return mpf(1)
    f = f32(x)
    e = mpmath.floor(mpmath.log(abs(f), 2))
    half_ulp = mpf(2) ** (e - 24)
    return (half_ulp - abs(x - f)) / abs(x)


# ---- small helpers
def norm3(w):
    return mpmath.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])


def hat(w):
    return [mpf(0), -w[2], w[1], w[2], mpf(0), -w[0], -w[1], w[0], mpf(0)]


def mm3(A, B):
    return [A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j] for i in range(3) for j in range(3)]


def mv3(A, v):
    return [A[i * 3] * v[0] + A[i * 3 + 1] * v[1] + A[i * 3 + 2] * v[2] for i in range(3)]


def eye3():
    return [mpf(1), mpf(0), mpf(0), mpf(0), mpf(1), mpf(0), mpf(0), mpf(0), mpf(1)]


def q_mul(a, b):
    """Eigen's quaternion product, (w, x, y, z)"""
    return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
            a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
            a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]]


def q_norm(q):
    n = mpmath.sqrt(sum(t * t for t in q))
    return [t / n for t in q]


def quat_to_R(q):
    """Eigen's toRotationMatrix, row-major; for a unit quaternion this is the rotation matrix itself"""
    w, x, y, z = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx,
            txz - twy, tyz + twx, 1 - (txx + tyy)]


def R_to_q_branch(R):
    """which case of Eigen's Quaternion(Matrix3) a matrix takes: 'trace' or the i of the largest diagonal entry"""
    if R[0] + R[4] + R[8] > 0:
        return "trace"
    i = 0
    if R[4] > R[0]:
        i = 1
    if R[8] > R[i * 3 + i]:
        i = 2
    return i


def R_to_q_aw(R):
    """Eigen::Quaternion(Matrix3) followed by normalize(), as SO3ex(R) does (so3_extra.h:60-64)"""
    t = R[0] + R[4] + R[8]
    if t > 0:
        t = mpmath.sqrt(t + 1)
        w = t / 2
        t = mpf(1) / 2 / t
        q = [w, (R[7] - R[5]) * t, (R[2] - R[6]) * t, (R[3] - R[1]) * t]
    else:
        i = R_to_q_branch(R)
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = mpmath.sqrt(R[i * 3 + i] - R[j * 3 + j] - R[k * 3 + k] + 1)
        v = [None] * 3
        v[i] = t / 2
        t = mpf(1) / 2 / t
        w = (R[k * 3 + j] - R[j * 3 + k]) * t
        v[j] = (R[j * 3 + i] + R[i * 3 + j]) * t
        v[k] = (R[k * 3 + i] + R[i * 3 + k]) * t
        q = [w] + v
    return q_norm(q)


# ---- SO(3), common/so3_extra.h
def so3_exp_aw(w):
    """SO3ex::exp, so3_extra.h:121-142, and the normalising constructor :70-76"""
    th = norm3(w)
    if th < SMALL_EPS:
        t2 = th * th
        imag, real = mpf(1) / 2 - t2 / 48, 1 - t2 / 8
    else:
        imag, real = mpmath.sin(th / 2) / th, mpmath.cos(th / 2)
    return q_norm([real, imag * w[0], imag * w[1], imag * w[2]])


def so3_exp_ex(w):
    th = norm3(w)
    if th == 0:
        return [mpf(1), mpf(0), mpf(0), mpf(0)]
    s = mpmath.sin(th / 2) / th
    return [mpmath.cos(th / 2), s * w[0], s * w[1], s * w[2]]


def so3_log_branch(q):
    n = norm3(q[1:])
    if n < SMALL_EPS:
        return "n<eps"
    if abs(q[0]) < SMALL_EPS:
        return "w>0" if q[0] > 0 else "w<=0"
    return "atan"


def so3_log_aw(q):
    """SO3ex::log, so3_extra.h:152-190"""
    n, w = norm3(q[1:]), q[0]
    sw = w * w
    b = so3_log_branch(q)
    if b == "n<eps":
        f = 2 / w - mpf(2) / 3 * (n * n) / (w * sw)
    elif b == "atan":
        f = 2 * mpmath.atan(n / w) / n
    else:
        f = (M_PI if b == "w>0" else -M_PI) / n
        n2 = n * n
        f -= 2 * w / n2 - mpf(2) / 3 * (w * sw) / (n2 * n2)
    return [f * q[1], f * q[2], f * q[3]]


def so3_log_ex(q):
    """theta = 2 atan(n / w) in [-pi, pi) (so3_extra.h:143-151, :178-180: w = 0 is -pi), times the unit axis"""
    n, w = norm3(q[1:]), q[0]
    if n == 0:
        return [mpf(0)] * 3
    th = 2 * mpmath.atan(n / w) if w != 0 else -mp.pi
    return [th / n * q[1], th / n * q[2], th / n * q[3]]


def so3_Jr_aw(w):
    """SO3ex::JacobianR, so3_extra.h:254-270"""
    th = norm3(w)
    if th < SMALL_EPS:
        O = hat(w)
        O2 = mm3(O, O)
        return [e - O[i] / 2 + O2[i] / 6 for i, e in enumerate(eye3())]
    K = hat([t / th for t in w])
    K2 = mm3(K, K)
    a, b = (1 - mpmath.cos(th)) / th, 1 - mpmath.sin(th) / th
    return [e - a * K[i] + b * K2[i] for i, e in enumerate(eye3())]


def so3_JrInv_aw(w):
    """SO3ex::JacobianRInv, so3_extra.h:271-288"""
    th = norm3(w)
    O = hat(w)
    if th < SMALL_EPS:
        O2 = mm3(O, O)
        return [e + O[i] / 2 + O2[i] / 12 for i, e in enumerate(eye3())]
    K = hat([t / th for t in w])
    K2 = mm3(K, K)
    c = 1 - (1 + mpmath.cos(th)) * th / (2 * mpmath.sin(th))
    return [e + O[i] / 2 + c * K2[i] for i, e in enumerate(eye3())]


def so3_Jr_ex(w):
    """the right Jacobian as its power series, sum_k (-hat(w))^k / (k + 1)!"""
    O = [-t for t in hat(w)]
    term, J, k = eye3(), eye3(), 0
    while True:
        k += 1
        term = [t / (k + 1) for t in mm3(term, O)]
        J = [a + b for a, b in zip(J, term)]
        if max(abs(t) for t in term) < mpf(10) ** -48:
            return J


def so3_JrInv_ex(w):
    J = so3_Jr_ex(w)
    return list(mpmath.inverse(mpmath.matrix([J[0:3], J[3:6], J[6:9]])))


# ---- retractions, src/Odom/NavState.h
def inc_small_pr_aw(p, q, d):
    """NavState::IncSmall(dPR) with USE_P_PLUS_RDP, NavState.h:47-58: p += Rwb dp; Rwb *= Exp(dphi), whose
    operator*= normalises (so3_extra.h:96-100)"""
    Rd = mv3(quat_to_R(q), d[0:3])
    return [p[i] + Rd[i] for i in range(3)], q_norm(q_mul(q, so3_exp_aw(d[3:6])))


def inc_small_pr_ex(p, q, d):
    Rd = mv3(quat_to_R(q), d[0:3])
    return [p[i] + Rd[i] for i in range(3)], q_norm(q_mul(q, so3_exp_ex(d[3:6])))


def ns_inc_aw(p, v, q, dbg, dba, d9, db6):
    """NavState::IncSmall(dPVR) and IncSmallBias, NavState.h:64-83"""
    Rd = mv3(quat_to_R(q), d9[0:3])
    return ([p[i] + Rd[i] for i in range(3)], [v[i] + d9[3 + i] for i in range(3)],
            q_norm(q_mul(q, so3_exp_aw(d9[6:9]))), [dbg[i] + db6[i] for i in range(3)],
            [dba[i] + db6[3 + i] for i in range(3)])


# ---- cameras, common/camera_models/camera_{pinhole,radtan,kb8}.h.  A camera is a dict: model (0 pinhole, 1 Radtan,
# 2 KB8), num_k, fx, fy, cx, cy and dist[8], all of them the floats the reference holds (Tdata), widened.
def _cam(c):
    return (mpf(float(c["fx"])), mpf(float(c["fy"])), mpf(float(c["cx"])), mpf(float(c["cy"])),
            [mpf(float(t)) for t in c["dist"]])


def kb8_project_branch(c, P):
    return "regular" if mpmath.sqrt(P[0] * P[0] + P[1] * P[1]) > PRECISION_R else "pinhole"


def cam_project_aw(c, P, rounded=True):
    """Project of the camera's model: (image point as the float Vec2data holds, or unrounded; the 2 x 3 Jacobian).
    camera_pinhole.h:70-106, camera_radtan.h:61-129, camera_kb8.h:68-157"""
    fx, fy, cx, cy, k = _cam(c)
    r_ = f32 if rounded else (lambda t: t)
    x, y, z = P
    if c["model"] == 1:
        nk = int(c["num_k"])
        p = k[nk:nk + 2]
        invz = 1 / z
        xn, yn = x * invz, y * invz
        x2, y2, xy = xn * xn, yn * yn, xn * yn
        r2 = x2 + y2
        fd, term = mpf(1), mpf(1)
        for i in range(nk):
            term *= r2
            fd += k[i] * term
        fd2, coeff2, term = mpf(0), mpf(0), mpf(1)
        for i in range(2, nk):          # camera_radtan.h:84-90: starts at k[2]
            coeff2 += 2
            fd2 += coeff2 * k[i] * term
            term *= r2
        # 3 * p[i] is an int times a Tdata: a float product, rounded to float (camera_radtan.h:91, :95)
        p0x3, p1x3 = f32(3 * p[0]), f32(3 * p[1])
        du_dx = fx * invz * (fd + fd2 * x2 + 2 * (p[0] * yn + p1x3 * xn))
        du_dy = fx * invz * (fd2 * xy + 2 * (p[0] * xn + p[1] * yn))
        du_dz = -(xn * du_dx + yn * du_dy)
        dv_dx = du_dy * fy / fx
        dv_dy = fy * invz * (fd + fd2 * y2 + 2 * (p[1] * xn + p0x3 * yn))
        dv_dz = -(xn * dv_dx + yn * dv_dy)
        xd = xn * fd + 2 * p[0] * xy + p[1] * (r2 + 2 * x2)
        yd = yn * fd + 2 * p[1] * xy + p[0] * (r2 + 2 * y2)
        return [r_(fx * xd + cx), r_(fy * yd + cy)], [du_dx, du_dy, du_dz, dv_dx, dv_dy, dv_dz]
    if c["model"] == 2 and kb8_project_branch(c, P) == "regular":
        x2, y2 = x * x, y * y
        r2 = x2 + y2
        r = mpmath.sqrt(r2)
        th = mpmath.atan2(r, z)
        t2 = th * th
        thd = th * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + k[3] * t2))))
        uv = [r_(fx * (x * thd / r) + cx), r_(fy * (y * thd / r) + cy)]
        invr = 1 / r
        tmp = 1 / (z * z + r2)
        dtx, dty = x * invr * z * tmp, y * invr * z * tmp
        dd = 1 + t2 * (3 * k[0] + t2 * (5 * k[1] + t2 * (7 * k[2] + 9 * k[3] * t2)))
        invr2 = invr * invr
        J01 = fx * x * (dd * dty * r - y * thd / r) * invr2
        return uv, [fx * (x * r * dd * dtx + y2 * thd / r) * invr2, J01, -fx * x * dd * tmp,
                    J01 * fy / fx, fy * (y * r * dd * dty + x2 * thd / r) * invr2, -fy * y * dd * tmp]
    invz = 1 / z
    return ([r_(fx * x * invz + cx), r_(fy * y * invz + cy)],
            [fx * invz, mpf(0), -fx * x * invz * invz, mpf(0), fy * invz, -fy * y * invz * invz])


def cam_project_ex(c, P):
    """the model's projection itself: no rounding, no degenerate branch (KB8 on the axis is its limit, the pinhole)"""
    fx, fy, cx, cy, k = _cam(c)
    x, y, z = P
    if c["model"] == 2:
        r = mpmath.sqrt(x * x + y * y)
        if r == 0:
            return [cx, cy]
        th = mpmath.atan2(r, z)
        t2 = th * th
        thd = th * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + k[3] * t2))))
        return [fx * x * thd / r + cx, fy * y * thd / r + cy]
    if c["model"] == 1:
        return cam_project_aw(c, P, rounded=False)[0]
    return [fx * x / z + cx, fy * y / z + cy]


def cam_project_J_ex(c, P):
    """d(u, v)/dP of cam_project_ex by central differences at h = 1e-15"""
    J = [None] * 6
    for a in range(3):
        Pp, Pm = list(P), list(P)
        Pp[a] += H_FD
        Pm[a] -= H_FD
        up, um = cam_project_ex(c, Pp), cam_project_ex(c, Pm)
        J[a], J[3 + a] = (up[0] - um[0]) / (2 * H_FD), (up[1] - um[1]) / (2 * H_FD)
    return J


def unproject_pinhole_aw(c, u, v):
    """PinholeCamera::UnProject to the plane z = 1, camera_pinhole.h:108-126"""
    fx, fy, cx, cy, _ = _cam(c)
    return [(u - cx) / fx, (v - cy) / fy, mpf(1)]


def cam_unproject_aw(c, u, v, info=None):
    """UnProject of the camera's model with kUnProject2Plane; u, v are floats.  camera_radtan.h:132-178,
    camera_kb8.h:159-195 with SolveTheta :278-312.  info (a dict) receives the branch taken and the iteration count."""
    info = {} if info is None else info
    fx, fy, cx, cy, k = _cam(c)
    t = unproject_pinhole_aw(c, u, v)
    if c["model"] == 1:
        y0, y1 = t[0], t[1]
        yb0, yb1 = y0, y1
        info["iterations"], info["min_inner_margin"] = MAX_ITER, mpf(1)
        for it in range(MAX_ITER):
            uv, J = cam_project_aw(c, [yb0, yb1, mpf(1)])
            raw = cam_project_aw(c, [yb0, yb1, mpf(1)], rounded=False)[0]
            info["min_inner_margin"] = min([info["min_inner_margin"]] + [f32_margin(t) for t in raw])
            tt = unproject_pinhole_aw(c, uv[0], uv[1])
            F00, F01, F11 = J[0] / fx, J[1] / fx, J[4] / fy
            F10 = F01                                        # camera_radtan.h:161
            e0, e1 = y0 - tt[0], y1 - tt[1]
            A00, A01, A11 = F00 * F00 + F10 * F10, F00 * F01 + F10 * F11, F01 * F01 + F11 * F11
            det = A00 * A11 - A01 * A01
            I00, I01, I11 = A11 / det, -A01 / det, A00 / det
            yb0 += (I00 * F00 + I01 * F01) * e0 + (I00 * F10 + I01 * F11) * e1
            yb1 += (I01 * F00 + I11 * F01) * e0 + (I01 * F10 + I11 * F11) * e1
            if e0 * e0 + e1 * e1 < PRECISION * PRECISION:
                info["iterations"] = it + 1
                break
        info["unrounded"] = [yb0, yb1]
        return [f32(yb0), f32(yb1), mpf(1)]
    if c["model"] == 2:
        mx, my = t[0], t[1]
        thd = mpmath.sqrt(mx * mx + my * my)
        half_pi = mpf(math.pi / 2.)                           # M_PI / 2., a double
        info["clamped"] = thd > half_pi
        thd = min(max(-half_pi, thd), half_pi)
        scaling = mpf(1)
        info["branch"] = "solve" if thd > PRECISION else "axis"
        if thd > PRECISION:
            th = thd
            info["iterations"] = MAX_ITER
            for it in range(MAX_ITER):
                t2 = th * th
                func = th * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + k[3] * t2))))
                # 9 * k4, 7 * k3, 5 * k2, 3 * k1 are int times Tdata: float products (camera_kb8.h:297-303)
                d = 1 + t2 * (f32(3 * k[0]) + t2 * (f32(5 * k[1]) + t2 * (f32(7 * k[2]) + f32(9 * k[3]) * t2)))
                fix = (thd - func) / d
                th += fix
                if abs(fix) < PRECISION:
                    info["iterations"] = it + 1
                    break
            info["theta"] = th
            scaling = mpmath.tan(th) / thd
        return [mx * scaling, my * scaling, mpf(1)]
    return t


# ---- inertial and encoder edges, src/Odom/g2otypes.h
def transpose3(A):
    return [A[j * 3 + i] for i in range(3) for j in range(3)]


def q_conj(q):
    return [q[0], -q[1], -q[2], -q[3]]


def imu_error_aw(M, gw, si, sj, idR):
    """EdgeNavStateI<NV>::computeError, g2otypes.h:725-771.  M: dict of the pre-integrated measurement (dt, Rij, vij,
    pij, JgR, Jgv, Jav, Jgp, Jap); si / sj: dicts p, v, q, dbg, dba.  Rows: e_p, then e_R at idR and e_v at 9 - idR.
    SO3ex(Rij) is Eigen's Quaternion(Matrix3) normalised (so3_extra.h:60-64), every SO3ex product normalises (:96-100)."""
    dt = M["dt"]
    RiT = transpose3(quat_to_R(si["q"]))
    t = [sj["p"][k] - si["p"][k] - si["v"][k] * dt - gw[k] * (dt * dt / 2) for k in range(3)]
    a, Jb, Ja = mv3(RiT, t), mv3(M["Jgp"], si["dbg"]), mv3(M["Jap"], si["dba"])
    e_p = [a[k] - (M["pij"][k] + Jb[k] + Ja[k]) for k in range(3)]
    t = [sj["v"][k] - si["v"][k] - gw[k] * dt for k in range(3)]
    a, Jb, Ja = mv3(RiT, t), mv3(M["Jgv"], si["dbg"]), mv3(M["Jav"], si["dba"])
    e_v = [a[k] - (M["vij"][k] + Jb[k] + Ja[k]) for k in range(3)]
    qa = q_norm(q_mul(R_to_q_aw(M["Rij"]), so3_exp_aw(mv3(M["JgR"], si["dbg"]))))
    qb = q_norm(q_mul(q_norm(q_conj(si["q"])), sj["q"]))
    e_R = so3_log_aw(q_norm(q_mul(q_norm(q_conj(qa)), qb)))
    err = [None] * 9
    err[0:3], err[idR:idR + 3], err[9 - idR:12 - idR] = e_p, e_R, e_v
    return err


def imu_error_ex(M, gw, si, sj, idR):
    """the residual with the exact exp and log"""
    dt = M["dt"]
    RiT = transpose3(quat_to_R(si["q"]))
    t = [sj["p"][k] - si["p"][k] - si["v"][k] * dt - gw[k] * (dt * dt / 2) for k in range(3)]
    a, Jb, Ja = mv3(RiT, t), mv3(M["Jgp"], si["dbg"]), mv3(M["Jap"], si["dba"])
    e_p = [a[k] - (M["pij"][k] + Jb[k] + Ja[k]) for k in range(3)]
    t = [sj["v"][k] - si["v"][k] - gw[k] * dt for k in range(3)]
    a, Jb, Ja = mv3(RiT, t), mv3(M["Jgv"], si["dbg"]), mv3(M["Jav"], si["dba"])
    e_v = [a[k] - (M["vij"][k] + Jb[k] + Ja[k]) for k in range(3)]
    qa = q_mul(R_to_q_aw(M["Rij"]), so3_exp_ex(mv3(M["JgR"], si["dbg"])))
    e_R = so3_log_ex(q_norm(q_mul(q_conj(qa), q_mul(q_conj(si["q"]), sj["q"]))))
    err = [None] * 9
    err[0:3], err[idR:idR + 3], err[9 - idR:12 - idR] = e_p, e_R, e_v
    return err


def _set3(J, ld, r0, c0, B, s=1):
    for i in range(3):
        for j in range(3):
            J[(r0 + i) * ld + c0 + j] = s * B[i * 3 + j]


def imu_linearize_aw(M, gw, si, sj, err, idR):
    """EdgeNavStateI<NV>::linearizeOplus with USE_P_PLUS_RDP, g2otypes.h:772-884.  9 x 24, row-major: columns 0..8 the
    state j, 9..17 the state i (each p, R at idR, V at idV = 9 - idR), 18..23 the bias of i."""
    idV = 9 - idR
    dt = M["dt"]
    J = [mpf(0)] * (9 * 24)
    cj, ci, cb = 0, 9, 18
    RiT = transpose3(quat_to_R(si["q"]))
    Rj = quat_to_R(sj["q"])
    t = [sj["p"][k] - si["p"][k] - si["v"][k] * dt - gw[k] * (dt * dt / 2) for k in range(3)]
    _set3(J, 24, 0, ci + idR, hat(mv3(RiT, t)))
    _set3(J, 24, 0, ci, eye3(), -1)
    _set3(J, 24, 0, ci + idV, RiT, -dt)
    _set3(J, 24, 0, cb, M["Jgp"], -1)
    _set3(J, 24, 0, cb + 3, M["Jap"], -1)
    _set3(J, 24, 0, cj, mm3(RiT, Rj))
    t = [sj["v"][k] - si["v"][k] - gw[k] * dt for k in range(3)]
    _set3(J, 24, idV, ci + idR, hat(mv3(RiT, t)))
    _set3(J, 24, idV, ci + idV, RiT, -1)
    _set3(J, 24, idV, cb, M["Jgv"], -1)
    _set3(J, 24, idV, cb + 3, M["Jav"], -1)
    _set3(J, 24, idV, cj + idV, RiT)
    eR = err[idR:idR + 3]
    Jrinv = so3_JrInv_aw(eR)
    Rji = quat_to_R(q_norm(q_mul(q_norm(q_conj(sj["q"])), si["q"])))
    _set3(J, 24, idR, ci + idR, mm3(Jrinv, Rji), -1)
    E = quat_to_R(so3_exp_aw([-t for t in eR]))
    Jr = so3_Jr_aw(mv3(M["JgR"], si["dbg"]))
    _set3(J, 24, idR, cb, mm3(mm3(mm3(Jrinv, E), Jr), M["JgR"]), -1)
    _set3(J, 24, idR, cj + idR, Jrinv)
    return J


def prior_error_aw(pr, si):
    """EdgeNavStatePriorPVRBias::computeError with USE_P_PLUS_RDP, g2otypes.cpp:84-108.  pr (the measurement) and si:
    dicts p, v, q, bg, ba, dbg, dba.  Rows: e_p = Rbw_bar (p - p_bar), e_v, e_R = Log(Rbw_bar Rwb), e_bg, e_ba.
    mRwb.inverse() is the conjugate, normalised by the constructor (so3_extra.h:105, :70-76), every SO3ex product
    normalises (:96-100), and SO3ex * vector is Eigen's _transformVector (:102-104), which for a unit quaternion is the
    rotation matrix times the vector."""
    qbw = q_norm(q_conj(pr["q"]))
    e_p = mv3(quat_to_R(qbw), [si["p"][k] - pr["p"][k] for k in range(3)])
    e_R = so3_log_aw(q_norm(q_mul(qbw, si["q"])))
    e_v = [si["v"][k] - pr["v"][k] for k in range(3)]
    e_bg = [si["bg"][k] + si["dbg"][k] - (pr["bg"][k] + pr["dbg"][k]) for k in range(3)]
    e_ba = [si["ba"][k] + si["dba"][k] - (pr["ba"][k] + pr["dba"][k]) for k in range(3)]
    return e_p + e_v + e_R + e_bg + e_ba


def prior_error_ex(pr, si):
    """the residual with the exact log"""
    qbw = q_norm(q_conj(pr["q"]))
    e = prior_error_aw(pr, si)
    e[6:9] = so3_log_ex(q_norm(q_mul(qbw, si["q"])))
    return e


def prior_linearize_aw(pr, si, err):
    """EdgeNavStatePriorPVRBias::linearizeOplus with USE_P_PLUS_RDP, g2otypes.cpp:109-124, as one 15 x 15 matrix,
    row-major: columns 0..8 the PVR vertex (dp, dv, dphi), 9..14 the bias vertex.  getRwb() is the matrix of the
    SO3ex's quaternion, which its constructors have normalised (so3_extra.h:60-76, :106)."""
    J = [mpf(0)] * 225
    _set3(J, 15, 0, 0, mm3(transpose3(quat_to_R(q_norm(pr["q"]))), quat_to_R(q_norm(si["q"]))))
    _set3(J, 15, 3, 3, eye3())
    _set3(J, 15, 6, 6, so3_JrInv_aw(err[6:9]))
    _set3(J, 15, 9, 9, eye3())
    _set3(J, 15, 12, 12, eye3())
    return J


def jrinv_g_ex(t):
    """the coefficient of hat(e)^2 in JacobianRInv(e), |e| = t: g = (1 - t (1 + cos t) / (2 sin t)) / t^2 (1 / 12 at 0)"""
    t = mpf(t)
    if t == 0:
        return mpf(1) / 12
    return (1 - t * (1 + mpmath.cos(t)) / (2 * mpmath.sin(t))) / (t * t)


def atan_PQ_ex(x2):
    """P = atan(x) / x and Q = (1 - P) / x^2 for x^2 = x2 >= 0 (1 and 1 / 3 at 0)"""
    x2 = mpf(x2)
    if x2 == 0:
        return mpf(1), mpf(1) / 3
    x = mpmath.sqrt(x2)
    P = mpmath.atan(x) / x
    return P, (1 - P) / x2


def solve_shifted_ex(H, lam, b):
    """x of (H + lam I) x = b in 50 digits; H: n x n floats, row-major rows"""
    n = len(b)
    A = mpmath.matrix(n, n)
    for i in range(n):
        for j in range(n):
            A[i, j] = mpf(float(H[i][j])) + (mpf(float(lam)) if i == j else 0)
    return list(mpmath.lu_solve(A, mpmath.matrix([mpf(float(t)) for t in b])))


def enc_edge_aw(si, sj, meas, qbe, pbe):
    """EdgeEncNavState<DV>::computeError / linearizeOplus with USE_P_PLUS_RDP, g2otypes.h:606-665: err = (e_R, e_p),
    Ji / Jj 6 x 6 with columns (dp, dphi)"""
    qi, qj = si["q"], sj["q"]
    qRiw, qReb = q_norm(q_conj(qi)), q_conj(qbe)
    qRij = q_mul(qRiw, qj)
    qe = q_norm(q_mul(q_mul(qReb, qRij), qbe))
    ql = q_norm(q_mul(q_norm(q_conj(so3_exp_aw(meas[0:3]))), qe))
    eR = so3_log_aw(ql)
    Riw, Rij, Reb = quat_to_R(qRiw), quat_to_R(qRij), quat_to_R(qReb)
    dpw = [sj["p"][k] - si["p"][k] for k in range(3)]
    a, b = mv3(Riw, dpw), mv3(Rij, pbe)
    dp = mv3(Reb, [a[k] - pbe[k] + b[k] for k in range(3)])
    err = eR + [dp[k] - meas[3 + k] for k in range(3)]
    Ji, Jj = [mpf(0)] * 36, [mpf(0)] * 36
    Jrinv = so3_JrInv_aw(eR)
    _set3(Ji, 6, 0, 3, mm3(mm3(Jrinv, Reb), transpose3(Rij)), -1)
    RebRiw = quat_to_R(q_mul(qReb, qRiw))
    _set3(Ji, 6, 3, 0, mm3(RebRiw, quat_to_R(qi)), -1)
    _set3(Ji, 6, 3, 3, mm3(Reb, hat([b[k] + a[k] for k in range(3)])))
    _set3(Jj, 6, 0, 3, mm3(Jrinv, Reb))
    _set3(Jj, 6, 3, 0, mm3(RebRiw, quat_to_R(qj)))
    _set3(Jj, 6, 3, 3, mm3(quat_to_R(q_mul(qReb, qRij)), hat(pbe)), -1)
    return err, Ji, Jj


# ---- the reprojection edge, src/Odom/g2otypes.h:321-547
def edge_xf_aw(c, p, q):
    """GetTcw_wX, g2otypes.h:359-369: Rcw = Rcb Rwb^T, tcw = -(Rcw twb) + tcb; c carries Rcb (9) and tcb (3)"""
    Rwb = quat_to_R(q)
    Rcw = mm3(V(c["Rcb"]), transpose3(Rwb))
    t = mv3(Rcw, p)
    return Rcw, [-t[k] + mpf(float(c["tcb"][k])) for k in range(3)], Rwb


def edge_eval_aw(c, bf, p, q, Xw, obs, info):
    """EdgeReproject::computeError (g2otypes.h:400-406, cam_project :338-345: the image point is the float the camera
    returns) and linearizeOplus with USE_P_PLUS_RDP (:439-498).  obs = (u, v, ur), stereo when ur >= 0.
    Returns chi2, err[3], Pc[3], J[3 x 6] (columns dp, dphi; for a monocular edge the third row is not the edge's),
    and the unrounded image point for the float excuse."""
    Rcw, tcw, Rwb = edge_xf_aw(c, p, q)
    a = mv3(Rcw, Xw)
    Pc = [a[k] + tcw[k] for k in range(3)]
    uv, Jc = cam_project_aw(c, Pc)
    raw = cam_project_aw(c, Pc, rounded=False)[0]
    stereo = obs[2] >= 0
    err = [obs[0] - uv[0], obs[1] - uv[1], obs[2] - (uv[0] - bf / Pc[2]) if stereo else mpf(0)]
    chi2 = sum(e * (info * e) for e in err)
    invz2 = 1 / (Pc[2] * Pc[2])
    Jp = [-t for t in Jc] + [-Jc[0], -Jc[1], -Jc[2] - bf * invz2]
    Rcb = V(c["Rcb"])
    JdP = mm3(Jp, [-t for t in Rcb])
    Paux = mv3(transpose3(Rwb), [Xw[k] - p[k] for k in range(3)])
    JdR = mm3(mm3(Jp, Rcb), hat(Paux))
    J = []
    for r in range(3):
        J += JdP[r * 3:r * 3 + 3] + JdR[r * 3:r * 3 + 3]
    return chi2, err, Pc, J, raw


def huber_aw(e, delta, dsqr):
    """RobustKernelHuber::robustify, robust_kernel_impl.cpp:78-91: rho, rho' and the branch"""
    if e <= dsqr:
        return [e, mpf(1)], "quadratic"
    sq = mpmath.sqrt(e)
    return [2 * sq * delta - dsqr, delta / sq], "linear"


def accumulate_aw(J, err, info, r1, stereo):
    """BaseMultiEdge::constructQuadraticForm for one vertex: the 21 upper entries of J^T (rho' Omega) J, row by row,
    and the 6 of -J^T rho' Omega e"""
    rows = 3 if stereo else 2
    w = r1 * info
    acc = []
    for a in range(6):
        for b in range(a, 6):
            acc.append(sum(J[r * 6 + a] * w * J[r * 6 + b] for r in range(rows)))
    return acc + [sum(J[r * 6 + a] * (-(info * err[r]) * r1) for r in range(rows)) for a in range(6)]


# ---- triangulation, common/camera_models/camera_base.h
def null_vector4_ex(A):
    """the right singular vector of the smallest singular value of A (rows of 4), which Eigen::JacobiSVD's
    matrixV().col(3) is (camera_base.h:599-600), by mpmath.svd_r; its sign is not the text's.  Also the two smallest
    singular values and the largest, for the vector's conditioning."""
    M = mpmath.matrix([list(r) for r in A])
    _, S, Vt = mpmath.svd_r(M)
    return [Vt[3, c] for c in range(4)], (S[3], S[2], S[0])


def triangulate_aw(obs, thresh, just_check_p3d, x3d, info=None):
    """GeometricCamera::TriangulateMatches with pTwr and purbf (camera_base.h:199-285) and Triangulate (:576-608).
    obs: the slots the reference's vectors hold, each a dict cam, T (Tcw, 12 values row-major 3 x 4), n (UnProject of
    the key point, z = 1), u, v, sigma2, uright, bf (floats).  Returns the point, or None for the empty vector.
    info: 'why' and 'margin', the least relative distance of a float rounding or a gate from its boundary."""
    info = {} if info is None else info
    margin = [mpf(1)]
    n = len(obs)
    R = [[o["T"][0:3], o["T"][4:7], o["T"][8:11]] for o in obs]
    t = [[o["T"][3], o["T"][7], o["T"][11]] for o in obs]

    def done(why, X):
        info["why"], info["margin"] = why, min(margin)
        return X
    if thresh < 1:
        bret = True
        for i in range(n - 1):
            ni = obs[i]["n"]
            for j in range(i + 1, n):
                nj = obs[j]["n"]
                w = [sum(R[j][r][c] * nj[r] for r in range(3)) for c in range(3)]         # Twj.so3() * n_j
                v = [sum(R[i][r][c] * w[c] for c in range(3)) for r in range(3)]          # Twi.so3().inverse() * that
                raw = sum(a * b for a, b in zip(ni, v)) / (norm3(ni) * norm3(v))
                cosr = f32(raw)
                margin.append(f32_margin(raw))
                margin.append(abs(cosr - thresh))
                if cosr <= thresh:
                    bret = False
        if bret:
            return done("parallax", None)
    if not just_check_p3d:
        A = []
        for o, Ti in zip(obs, [o["T"] for o in obs]):
            A.append([o["n"][0] * Ti[8 + c] - Ti[c] for c in range(4)])
            A.append([o["n"][1] * Ti[8 + c] - Ti[4 + c] for c in range(4)])
        x4, sv = null_vector4_ex(A)
        info["sv"] = sv
        if x4[3] == 0 or abs(x4[3]) < mpf(10) ** -40 * max(abs(c) for c in x4):
            return done("x4", None)
        X = [x4[0] / x4[3], x4[1] / x4[3], x4[2] / x4[3]]
    else:
        X = list(x3d)
    for k, o in enumerate(obs):
        Pc = [sum(R[k][r][c] * X[c] for c in range(3)) + t[k][r] for r in range(3)]
        cz = f32(Pc[2])
        margin.append(abs(Pc[2]) / norm3(Pc))
        if cz <= 0:
            return done("depth", None)
        uv, _ = cam_project_aw(o["cam"], Pc)
        margin.append(min(f32_margin(x) for x in cam_project_aw(o["cam"], Pc, rounded=False)[0]))
        e0, e1 = f32(uv[0] - o["u"]), f32(uv[1] - o["v"])
        err2, th = f32(f32(e0 * e0) + f32(e1 * e1)), f32(mpf("5.991"))
        if o["uright"] != -1:
            u2 = f32(uv[0] - f32(o["bf"] / cz))
            e2 = f32(u2 - o["uright"])
            err2, th = f32(err2 + f32(e2 * e2)), f32(mpf("7.8"))
        lim = f32(th * o["sigma2"])
        margin.append(abs(err2 - lim) / lim)
        if err2 > lim:
            return done("chi2", None)
    return done("ok", X)
