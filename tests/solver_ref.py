"""50-digit statements of the lane functions of the relocalisation and loop-verification solvers, the reference of
tests/test_solver_algebra.py: PnPsolver (src/PnPsolver.cc:367-875: compute_pose and what it calls, Getuv, CheckInliers
at :293-319) and Sim3Solver (src/Sim3Solver.cc:220-373: ComputeSim3, CheckInliers, Project).  mpmath at 50 digits.  The
linear algebra is the definition (mp.eigsy, mp.svd_r, the least-squares minimiser through the singular triplets); the float
roundings the reference makes are made here (invZc, crP3D, the image points, the squared distances).  Where the
reference leaves a sign to cv::SVD (the principal directions of the control points) the library's convention is taken:
the component of largest magnitude positive."""
import math

import mpmath
import numpy as np
from mpmath import mp, mpf

from tests.algebra_ref import V, cam_project_aw, f32, f32_margin

mp.dps = 50

PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
EPS_DOUBLE = mpf(2) ** -52


def M(a, rows, cols):
    """a flat sequence of numbers as an mp matrix"""
    a = [mpf(float(t)) if not isinstance(t, mpf) else t for t in a]
    return mpmath.matrix([[a[r * cols + c] for c in range(cols)] for r in range(rows)])


def flat(A):
    return [A[r, c] for r in range(A.rows) for c in range(A.cols)]


# ---------------------------------------------------------------------------------------------------------------------
# the helpers
RANK_TOL = mpf(10) ** -25   # a singular value below this share of the largest is zero: 25 digits under the 50 carried


def lstsq(A, b):
    """the minimiser of |A x - b| for A (6 x nc) from the definition: x = sum of (u_i . b / s_i) v_i over the singular
    triplets of A; of smallest norm where A has no full column rank, as cv::solve(DECOMP_SVD) takes it (the reference's
    qr_solve, :805-875, has the same x at full rank).  (x, residual norm, rank)"""
    U, s, Vt = mpmath.svd_r(A)
    x = mpmath.matrix(A.cols, 1)
    rank = 0
    for i in range(A.cols):
        if s[i] > RANK_TOL * s[0]:
            rank += 1
            x += (sum(U[r, i] * b[r] for r in range(A.rows)) / s[i]) * Vt[i, :].T
    return [x[i] for i in range(A.cols)], mpmath.norm(A * x - b, 2), rank


def residual(A, b, x):
    r = A * mpmath.matrix([mpf(float(t)) for t in x]) - b
    return mpmath.norm(r, 2)


def jacobi_rot(a, b, g):
    """(t, cs, sn) of the rotation that annihilates g between the diagonals a and b: t the root of smaller magnitude of
    t^2 + 2 zeta t - 1 = 0, zeta = (b - a) / (2 g)"""
    zeta = (b - a) / (2 * g)
    t = (1 if zeta >= 0 else -1) / (abs(zeta) + mpmath.sqrt(1 + zeta * zeta))
    cs = 1 / mpmath.sqrt(1 + t * t)
    return [t, cs, cs * t]


def fix_sign(v):
    """the library's convention: the component of largest magnitude positive (the first of them at a tie)"""
    big = v[0]
    for t in v[1:]:
        if abs(t) > abs(big):
            big = t
    return [-t for t in v] if big < 0 else list(v)


def eig_desc(S):
    """eigenvalues of the symmetric S in descending order and the matrix of their eigenvectors (columns, sign fixed)"""
    n = S.rows
    w, Q = mpmath.eigsy(S)
    order = sorted(range(n), key=lambda k: -w[k])
    U = mpmath.matrix(n, n)
    for c, k in enumerate(order):
        col = fix_sign([Q[r, k] for r in range(n)])
        for r in range(n):
            U[r, c] = col[r]
    return [w[k] for k in order], U


def polar3(B):
    """R = U V^T of the SVD of B (estimate_R_and_t, :553-599) and the singular values, descending"""
    U, s, Vt = mpmath.svd_r(B)
    return U * Vt, [s[i] for i in range(3)]


def alphas(c0, ci, X):
    d = [X[k] - c0[k] for k in range(3)]
    a = [None] + [ci[j][0] * d[0] + ci[j][1] * d[1] + ci[j][2] * d[2] for j in range(3)]
    a[0] = 1 - a[1] - a[2] - a[3]
    return a


def getuv(K, R, t, X):
    """Getuv of the rectified configuration (:406-419): invZc is a float.  (ue, ve, margin of invZc's rounding)"""
    fx, fy, cx, cy = K
    P = [R[r][0] * X[0] + R[r][1] * X[1] + R[r][2] * X[2] + t[r] for r in range(3)]
    iz = 1 / P[2]
    invz = f32(iz)
    return cx + fx * P[0] * invz, cy + fy * P[1] * invz, f32_margin(iz)


def check_inlier(K, R, t, X, uv, max_err):
    """CheckInliers (:293-319) of one correspondence: (inlier, margin): the smallest relative distance of a value rounded
    from double arithmetic from its rounding boundary"""
    ue, ve, m0 = getuv(K, R, t, X)
    dx, dy = uv[0] - ue, uv[1] - ve
    fx_, fy_ = f32(dx), f32(dy)
    xx, yy = fx_ * fx_, fy_ * fy_
    s = f32(xx) + f32(yy)
    e2 = f32(s)
    # what follows the two float differences is arithmetic on floats, exact or rounded once from an exact value: the
    # same everywhere, ties included; only invZc and the differences come out of double arithmetic
    margins = [m0, f32_margin(dx), f32_margin(dy)]
    return e2 < max_err, min(margins)


# ---------------------------------------------------------------------------------------------------------------------
# compute_pose (:451-497)
def _pose_from_betas(betas, v, al, pw, us, K):
    """compute_R_and_t (:601-610): compute_ccs, compute_pcs, solve_for_sign, estimate_R_and_t, reprojection_error"""
    n = len(pw)
    ccs = [[sum(betas[i] * v[i][j][c] for i in range(4)) for c in range(3)] for j in range(4)]
    pcs = [[sum(al[i][j] * ccs[j][c] for j in range(4)) for c in range(3)] for i in range(n)]
    z0 = pcs[0][2]
    if z0 < 0:
        ccs = [[-t for t in row] for row in ccs]
        pcs = [[-t for t in row] for row in pcs]
    pc0 = [sum(p[c] for p in pcs) / n for c in range(3)]
    pw0 = [sum(p[c] for p in pw) / n for c in range(3)]
    ABt = mpmath.matrix(3, 3)
    for r in range(3):
        for c in range(3):
            ABt[r, c] = sum((pcs[i][r] - pc0[r]) * (pw[i][c] - pw0[c]) for i in range(n))
    R, sv = polar3(ABt)
    det = mpmath.det(R)
    if det < 0:
        for c in range(3):
            R[2, c] = -R[2, c]
    Rl = [[R[r, c] for c in range(3)] for r in range(3)]
    t = [pc0[r] - (Rl[r][0] * pw0[0] + Rl[r][1] * pw0[1] + Rl[r][2] * pw0[2]) for r in range(3)]
    err = mpf(0)
    for i in range(n):
        ue, ve, _ = getuv(K, Rl, t, pw[i])
        err += mpmath.sqrt((us[i][0] - ue) ** 2 + (us[i][1] - ve) ** 2)
    return err / n, Rl, t, z0, det, sv


def epnp(pw, us, K):
    """compute_pose over the correspondences pw (n, 3) / us (n, 2) (floats).  A dict: R (3 x 3 list), t, and what decides
    the branches: eig (the four smallest eigenvalues of MtM, smallest first, and the fifth), rho, x (the least-squares
    solutions of the three initial guesses), betas0, err, z0, det, sv (singular values of ABt), variant (0-based)."""
    pw = [V(p) for p in pw]
    us = [V(u) for u in us]
    K = V(K)
    fx, fy, cx, cy = K
    n = len(pw)
    # choose_control_points (:367-404)
    c0 = [sum(p[c] for p in pw) / n for c in range(3)]
    S = mpmath.matrix(3, 3)
    for r in range(3):
        for c in range(3):
            S[r, c] = sum((p[r] - c0[r]) * (p[c] - c0[c]) for p in pw)
    w, U = eig_desc(S)
    cws = [c0]
    ks = []
    for j in range(3):
        k = mpmath.sqrt(max(w[j], 0) / n)
        ks.append(k)
        cws.append([c0[r] + k * U[r, j] for r in range(3)])
    # compute_barycentric_coordinates (:406-425): CC^-1, the pseudo-inverse where a direction has no extent
    ci = [[(U[r, j] / ks[j] if ks[j] > 0 else mpf(0)) for r in range(3)] for j in range(3)]
    al = [alphas(c0, ci, p) for p in pw]
    # fill_M (:427-441), MtM and its eigenvectors (:466-474)
    Mm = mpmath.matrix(2 * n, 12)
    for i in range(n):
        for j in range(4):
            Mm[2 * i, 3 * j] = al[i][j] * fx
            Mm[2 * i, 3 * j + 2] = al[i][j] * (cx - us[i][0])
            Mm[2 * i + 1, 3 * j + 1] = al[i][j] * fy
            Mm[2 * i + 1, 3 * j + 2] = al[i][j] * (cy - us[i][1])
    wv, Q = mpmath.eigsy(Mm.T * Mm)
    order = sorted(range(12), key=lambda k: wv[k])
    v = [[[Q[3 * j + c, order[i]] for c in range(3)] for j in range(4)] for i in range(4)]
    # compute_L_6x10 (:612-649), compute_rho (:651-659)
    L = []
    for a, b in PAIRS:
        d = [[v[i][a][c] - v[i][b][c] for c in range(3)] for i in range(4)]
        dot = lambda p, q: d[p][0] * d[q][0] + d[p][1] * d[q][1] + d[p][2] * d[q][2]
        L.append([dot(0, 0), 2 * dot(0, 1), dot(1, 1), 2 * dot(0, 2), 2 * dot(1, 2), dot(2, 2), 2 * dot(0, 3), 2 * dot(1, 3),
                  2 * dot(2, 3), dot(3, 3)])
    rho = [sum((cws[a][c] - cws[b][c]) ** 2 for c in range(3)) for a, b in PAIRS]
    rho_v = mpmath.matrix(rho)

    def solve(cols, rhs):
        return lstsq(mpmath.matrix([[row[c] for c in cols] for row in L]), rhs)[0]

    def first_two(x):  # find_betas_approx_2 / 3 (:689-704, :729-746)
        if x[0] < 0:
            b0, b1 = mpmath.sqrt(-x[0]), (mpmath.sqrt(-x[2]) if x[2] < 0 else mpf(0))
        else:
            b0, b1 = mpmath.sqrt(x[0]), (mpmath.sqrt(x[2]) if x[2] > 0 else mpf(0))
        return (-b0 if x[1] < 0 else b0), b1

    xs, betas0 = [], []
    x = solve([0, 1, 3, 6], rho_v)  # find_betas_approx_1 (:661-687)
    sg = -1 if x[0] < 0 else 1
    b0 = mpmath.sqrt(sg * x[0])
    xs.append(x), betas0.append([b0, sg * x[1] / b0, sg * x[2] / b0, sg * x[3] / b0])
    x = solve([0, 1, 2], rho_v)
    b0, b1 = first_two(x)
    xs.append(x), betas0.append([b0, b1, mpf(0), mpf(0)])
    x = solve([0, 1, 2, 3, 4], rho_v)
    b0, b1 = first_two(x)
    xs.append(x), betas0.append([b0, b1, x[3] / b0, mpf(0)])

    def gauss_newton(b):  # :783-803, compute_A_and_b_gauss_newton (:748-781)
        b = list(b)
        for _ in range(5):
            A, r = mpmath.matrix(6, 4), mpmath.matrix(6, 1)
            for k, Lr in enumerate(L):
                A[k, 0] = 2 * Lr[0] * b[0] + Lr[1] * b[1] + Lr[3] * b[2] + Lr[6] * b[3]
                A[k, 1] = Lr[1] * b[0] + 2 * Lr[2] * b[1] + Lr[4] * b[2] + Lr[7] * b[3]
                A[k, 2] = Lr[3] * b[0] + Lr[4] * b[1] + 2 * Lr[5] * b[2] + Lr[8] * b[3]
                A[k, 3] = Lr[6] * b[0] + Lr[7] * b[1] + Lr[8] * b[2] + 2 * Lr[9] * b[3]
                r[k] = rho[k] - (Lr[0] * b[0] * b[0] + Lr[1] * b[0] * b[1] + Lr[2] * b[1] * b[1] + Lr[3] * b[0] * b[2] +
                                 Lr[4] * b[1] * b[2] + Lr[5] * b[2] * b[2] + Lr[6] * b[0] * b[3] + Lr[7] * b[1] * b[3] +
                                 Lr[8] * b[2] * b[3] + Lr[9] * b[3] * b[3])
            dx = lstsq(A, r)[0]
            b = [b[k] + dx[k] for k in range(4)]
        return b

    res = [_pose_from_betas(gauss_newton(b), v, al, pw, us, K) for b in betas0]
    N = 0
    if res[1][0] < res[0][0]:
        N = 1
    if res[2][0] < res[N][0]:
        N = 2
    return dict(R=res[N][1], t=res[N][2], eig=[wv[order[i]] for i in range(5)], rho=rho, x=xs, betas0=betas0,
                err=[r[0] for r in res], z0=[r[3] for r in res], det=[r[4] for r in res], sv=[r[5] for r in res], variant=N,
                cond_S=w)


# ---------------------------------------------------------------------------------------------------------------------
# Sim3Solver
def top_eigenvector(N):
    """the unit eigenvector of the largest eigenvalue of the symmetric 4 x 4 N (cv::eigen's row 0, :266-270), sign
    fixed, and the eigenvalues in descending order"""
    w, U = eig_desc(N)
    return [U[r, 0] for r in range(4)], w


def horn_n(P1, P2):
    """Steps 1-3 of ComputeSim3 (:226-263): N (full symmetric), O1, O2, Pr1, Pr2; a point per row"""
    O1 = [(P1[0][c] + P1[1][c] + P1[2][c]) / 3 for c in range(3)]
    O2 = [(P2[0][c] + P2[1][c] + P2[2][c]) / 3 for c in range(3)]
    Pr1 = [[P1[i][c] - O1[c] for c in range(3)] for i in range(3)]
    Pr2 = [[P2[i][c] - O2[c] for c in range(3)] for i in range(3)]
    m = [[sum(Pr2[i][a] * Pr1[i][b] for i in range(3)) for b in range(3)] for a in range(3)]
    N = mpmath.matrix(4, 4)
    N[0, 0], N[0, 1], N[0, 2], N[0, 3] = m[0][0] + m[1][1] + m[2][2], m[1][2] - m[2][1], m[2][0] - m[0][2], m[0][1] - m[1][0]
    N[1, 1], N[1, 2], N[1, 3] = m[0][0] - m[1][1] - m[2][2], m[0][1] + m[1][0], m[2][0] + m[0][2]
    N[2, 2], N[2, 3] = -m[0][0] + m[1][1] - m[2][2], m[1][2] + m[2][1]
    N[3, 3] = -m[0][0] - m[1][1] + m[2][2]
    for r in range(4):
        for c in range(r):
            N[r, c] = N[c, r]
    return N, O1, O2, Pr1, Pr2


def rodrigues(r):
    """cv::Rodrigues, vector -> matrix (theta below DBL_EPSILON: the identity)"""
    theta = mpmath.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    if theta < EPS_DOUBLE:
        return [[mpf(int(i == j)) for j in range(3)] for i in range(3)]
    c, s = mpmath.cos(theta), mpmath.sin(theta)
    x, y, z = (t / theta for t in r)
    c1 = 1 - c
    return [[c + c1 * x * x, c1 * x * y - s * z, c1 * x * z + s * y], [c1 * x * y + s * z, c + c1 * y * y, c1 * y * z - s * x],
            [c1 * x * z - s * y, c1 * y * z + s * x, c + c1 * z * z]]


def horn(P1, P2, fix_scale):
    """ComputeSim3 (:220-322) on 3 pairs (a point per row).  (R, t, s, info): info has q (the eigenvector), w (N's
    eigenvalues, descending), nv, theta, den; s is None where the reference divides by zero"""
    P1, P2 = [V(p) for p in P1], [V(p) for p in P2]
    N, O1, O2, Pr1, Pr2 = horn_n(P1, P2)
    q, w = top_eigenvector(N)
    nv = mpmath.sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    ang = mpmath.atan2(nv, q[0])
    if nv > 0:
        rv = [2 * ang * q[1 + k] / nv for k in range(3)]
    else:  # 0 / 0 in the reference; the library: the identity
        rv = [mpf(0)] * 3
    R = rodrigues(rv)
    den = None
    if not fix_scale:
        nom = den = mpf(0)
        for i in range(3):
            for r in range(3):
                p3 = R[r][0] * Pr2[i][0] + R[r][1] * Pr2[i][1] + R[r][2] * Pr2[i][2]
                nom += Pr1[i][r] * p3
                den += p3 * p3
        s = nom / den if den != 0 else None
    else:
        s = mpf(1)
    t = [O1[r] - s * (R[r][0] * O2[0] + R[r][1] * O2[1] + R[r][2] * O2[2]) for r in range(3)] if s is not None else None
    theta = mpmath.sqrt(sum(x * x for x in rv))
    return R, t, s, dict(q=q, w=w, nv=nv, theta=theta, den=den, N=N)


def sim3_pose(R, t, s):
    """Step 8 (:311-321): A12 = s R, t12 = t, A21 = R^T / s, t21 = -A21 t; 24 values in the order of the program"""
    A12 = [[s * R[r][c] for c in range(3)] for r in range(3)]
    A21 = [[R[c][r] / s for c in range(3)] for r in range(3)]
    t21 = [-(A21[r][0] * t[0] + A21[r][1] * t[1] + A21[r][2] * t[2]) for r in range(3)]
    return [x for row in A12 for x in row] + list(t) + [x for row in A21 for x in row] + t21


def sim3_project(cam, A, t, X):
    """Project (:352-373) of one point: crP3D = X, or A X + t rounded to float; Tcr of the camera; its model.
    (the two float image coordinates, margin: the smallest relative distance of a rounded value from its boundary)"""
    P = list(X)
    margin = mpf(1)
    if A is not None:
        Q = [A[r][0] * X[0] + A[r][1] * X[1] + A[r][2] * X[2] + t[r] for r in range(3)]
        margin = min(f32_margin(x) for x in Q)
        P = [f32(x) for x in Q]
    Rcb, tcb = V(cam["Rcb"]), V(cam["tcb"])
    Pc = [Rcb[3 * r] * P[0] + Rcb[3 * r + 1] * P[1] + Rcb[3 * r + 2] * P[2] + tcb[r] for r in range(3)]
    raw, _ = cam_project_aw(cam, Pc, rounded=False)
    margin = min([margin] + [f32_margin(x) for x in raw])
    return [f32(x) for x in raw], margin


def dist2(a, b):
    """dist.dot(dist) as a float (:333-340): float differences, their squares summed in double.  (value, margin)"""
    dx, dy = a[0] - b[0], a[1] - b[1]
    fx_, fy_ = f32(dx), f32(dy)
    s = fx_ * fx_ + fy_ * fy_        # double products of floats are exact; their sum is rounded to double first
    sd = mpf(float(s))
    return f32(sd), mpf(1)           # floats in, every step exact or rounded once from an exact value: no margin


def sim3_is_inlier(T24, cam1, cam2, X1, X2, me1, me2):
    """CheckInliers (:324-344) of one correspondence.  (inlier, margin)"""
    A12, t12 = [T24[3 * r:3 * r + 3] for r in range(3)], T24[9:12]
    A21, t21 = [T24[12 + 3 * r:15 + 3 * r] for r in range(3)], T24[21:24]
    p1im1, m1 = sim3_project(cam1, None, None, X1)
    p2im2, m2 = sim3_project(cam2, None, None, X2)
    p2im1, m3 = sim3_project(cam1, A12, t12, X2)
    p1im2, m4 = sim3_project(cam2, A21, t21, X1)
    e1, m5 = dist2(p1im1, p2im1)
    e2, m6 = dist2(p1im2, p2im2)
    return (e1 < me1 and e2 < me2), min([m1, m2, m3, m4, m5, m6])


def to_float(x):
    return float(x)


def pose_error(R, t, R0, t0):
    """(|t - t0|, the angle of R0^T R) in double, from mp inputs"""
    R = np.array([[float(x) for x in row] for row in R])
    R0 = np.array([[float(x) for x in row] for row in R0])
    D = R0.T @ R
    s = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.linalg.norm(np.array([float(a) - float(b) for a, b in zip(t, t0)]))), math.atan2(
        float(np.linalg.norm(s)), 0.5 * (np.trace(D) - 1.0))
