"""50-digit reference of the Sim3 algebra (vieo_slam_amd/csrc/sim3_device.h), written from the text of g2o's
types/sim3.h and of Eigen's quaternion <-> matrix conversions: every branch as written, taken on the quantity the code
tests (the trace and the diagonal in the conversion, theta and |sigma| in exp, d and |log s| in log), eps = 0.00001 the
double the text names, 1. / 2. and 1. / 6. the doubles the text names.  The 3 x 3 solve of log is stated from its
definition (W upsilon = t).  Nothing here rounds to a double: the inputs are doubles, everything else has 50 digits.

A second set of statements comes from exact definitions (exp_exact: the series of the 4 x 4 generator's exponential)
and is used only where the tests measure how far the text is from the exponential.

A Sim3 is a flat list [qx, qy, qz, qw, tx, ty, tz, s], as the device's struct lays it out."""
import mpmath
from mpmath import mpf

mpmath.mp.dps = 50

EPS = mpf(0.00001)        # `double eps = 0.00001`
HALF = mpf(1.0 / 2.0)
SIXTH = mpf(1.0 / 6.0)    # `1. / 6.`: the double


def V(x):
    return [mpf(float(t)) for t in x]


# ---------------------------------------------------------------------------------------- conversions
def quat_to_mat(q):
    """Eigen::QuaternionBase::toRotationMatrix, no normalisation"""
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)]


def mat_to_quat_branch(R):
    """(branch, trace): 0 for trace > 0, else 1 + i with i the largest diagonal entry as the text's two `>` find it"""
    t = R[0] + R[4] + R[8]
    if t > 0:
        return 0, t
    i = 0
    if R[4] > R[0]:
        i = 1
    if R[8] > R[4 * i]:
        i = 2
    return 1 + i, t


def mat_to_quat(R):
    """Eigen's quaternionbase_assign_impl<Other, 3, 3>"""
    br, t = mat_to_quat_branch(R)
    q = [mpf(0)] * 4
    if br == 0:
        t = mpmath.sqrt(t + 1)
        q[3] = t / 2
        t = HALF / t
        q[0], q[1], q[2] = (R[7] - R[5]) * t, (R[2] - R[6]) * t, (R[3] - R[1]) * t
    else:
        i = br - 1
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = mpmath.sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1)
        q[i] = t / 2
        t = HALF / t
        q[3] = (R[3 * k + j] - R[3 * j + k]) * t
        q[j] = (R[3 * j + i] + R[3 * i + j]) * t
        q[k] = (R[3 * k + i] + R[3 * i + k]) * t
    return q


def quat_mul(a, b):
    return [a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
            a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def quat_rot(q, v):
    """Eigen's _transformVector: v + w (2 q x v) + q x (2 q x v), no normalisation"""
    uv = [2 * c for c in _cross(q[:3], v)]
    c = _cross(q[:3], uv)
    return [v[i] + q[3] * uv[i] + c[i] for i in range(3)]


# ---------------------------------------------------------------------------------------- group operations
def mul(a, b):
    """sim3.h operator*: r = r1 r2, t = s1 (r1 t2) + t1, s = s1 s2"""
    r = quat_rot(a[0:4], b[4:7])
    return quat_mul(a[0:4], b[0:4]) + [a[7] * r[i] + a[4 + i] for i in range(3)] + [a[7] * b[7]]


def inverse(a):
    """sim3.h inverse(): (r*, r* ((-1 / s) t), 1 / s)"""
    qc = [-a[0], -a[1], -a[2], a[3]]
    m = -1 / a[7]
    return qc + quat_rot(qc, [m * a[4], m * a[5], m * a[6]]) + [1 / a[7]]


def smap(a, p):
    r = quat_rot(a[0:4], p)
    return [a[7] * r[i] + a[4 + i] for i in range(3)]


def _skew(w):
    z = mpf(0)
    return [z, -w[2], w[1], w[2], z, -w[0], -w[1], w[0], z]


def _mm(A, B):
    return [sum(A[3 * i + k] * B[3 * k + j] for k in range(3)) for i in range(3) for j in range(3)]


def _abc(sigma, s, theta, small_theta):
    """A, B, C of the text's four branches -> (A, B, C, sigma_small)"""
    if abs(sigma) < EPS:
        C = mpf(1)
        if small_theta:
            A, B = HALF, SIXTH
        else:
            theta2 = theta * theta
            A = (1 - mpmath.cos(theta)) / theta2
            B = (theta - mpmath.sin(theta)) / (theta2 * theta)
        return A, B, C, True
    C = (s - 1) / sigma
    if small_theta:
        sigma2 = sigma * sigma
        A = ((sigma - 1) * s + 1) / sigma2
        B = ((HALF * sigma2 - sigma + 1) * s - 1) / (sigma2 * sigma)
    else:
        a, b = s * mpmath.sin(theta), s * mpmath.cos(theta)
        theta2, sigma2 = theta * theta, sigma * sigma
        c = theta2 + sigma2
        A = (a * sigma + (1 - b) * theta) / (theta * c)
        B = (C - ((b - 1) * sigma + a * theta) / c) * 1 / theta2
    return A, B, C, False


def exp(u):
    """Sim3(const Vector7d&) -> (S[8], taps): taps = dict(theta, small_theta, sigma_small, m2q, trace)"""
    omega, upsilon, sigma = u[0:3], u[3:6], u[6]
    theta = mpmath.sqrt(omega[0] * omega[0] + omega[1] * omega[1] + omega[2] * omega[2])
    O = _skew(omega)
    O2 = _mm(O, O)
    s = mpmath.exp(sigma)
    small = theta < EPS
    eye = [mpf(1 if i % 4 == 0 else 0) for i in range(9)]
    if small:
        R = [eye[i] + O[i] + O2[i] / 2 for i in range(9)]
    else:
        a, b = mpmath.sin(theta) / theta, (1 - mpmath.cos(theta)) / (theta * theta)
        R = [eye[i] + a * O[i] + b * O2[i] for i in range(9)]
    A, B, C, sig_small = _abc(sigma, s, theta, small)
    W = [A * O[i] + B * O2[i] + C * eye[i] for i in range(9)]
    t = [sum(W[3 * i + j] * upsilon[j] for j in range(3)) for i in range(3)]
    br, tr = mat_to_quat_branch(R)
    return mat_to_quat(R) + t + [s], dict(theta=theta, small_theta=small, sigma_small=sig_small, m2q=br, trace=tr)


def log_taps(S):
    """the quantities log decides on, or None where acos leaves the reals (d outside [-1, 1])"""
    sigma = mpmath.log(S[7])
    R = quat_to_mat(S[0:4])
    d = HALF * (R[0] + R[4] + R[8] - 1)
    return dict(d=d, near_identity=d > 1 - EPS, sigma=sigma, sigma_small=abs(sigma) < EPS)


def log(S):
    """Sim3::log -> (res[7], taps); res is None where d lies outside [-1, 1] (acos is not real: the double code gives
    NaN there) or 1 - d^2 = 0"""
    T = log_taps(S)
    sigma, d = T["sigma"], T["d"]
    R = quat_to_mat(S[0:4])
    dR = [R[7] - R[5], R[2] - R[6], R[3] - R[1]]
    theta = mpf(0)
    if T["near_identity"]:
        omega = [HALF * v for v in dR]
    else:
        if d < -1 or d > 1 or d * d == 1:
            return None, T
        theta = mpmath.acos(d)
        f = theta / (2 * mpmath.sqrt(1 - d * d))
        omega = [f * v for v in dR]
    A, B, C, _ = _abc(sigma, S[7], theta, T["near_identity"])
    O = _skew(omega)
    O2 = _mm(O, O)
    W = mpmath.matrix(3, 3)
    for i in range(3):
        for j in range(3):
            W[i, j] = A * O[3 * i + j] + B * O2[3 * i + j] + (C if i == j else 0)
    ups = mpmath.lu_solve(W, mpmath.matrix(S[4:7]))
    return list(omega) + [ups[0], ups[1], ups[2]] + [sigma], T


def edge_error(C, Si, Sj):
    """EdgeSim3::computeError: log(C Si Sj^-1)"""
    return log(mul(mul(C, Si), inverse(Sj)))


# ---------------------------------------------------------------------------------------- OptimizeSim3's state
# (csrc/sim3_optimize_device.h, from Optimizer.cc:2689-2918 and NavState.h:47-58).  A state is [p[3], q[4], s].
def quat_normalize(q):
    n = mpmath.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return [c / n for c in q]


def state_from_sim3(R12, t12, s12):
    """mRwb = SO3exd(g2oS12.rotation()).inverse(), mpwb = -(mRwb * translation)"""
    q = quat_normalize(mat_to_quat(R12))
    qwb = quat_normalize([-q[0], -q[1], -q[2], q[3]])
    r = quat_rot(qwb, t12)
    return [-r[0], -r[1], -r[2]] + qwb + [s12]


def state_to_sim3(st):
    """R12 = mRwb.inverse(); Sim3(R12.unit_quaternion(), -(R12 * mpwb), scale) -> R12[9], t12[3], s12"""
    q = quat_normalize([-st[3], -st[4], -st[5], st[6]])
    r = quat_rot(q, st[0:3])
    return quat_to_mat(q) + [-r[0], -r[1], -r[2]] + [st[7]]


def inc_small(st, d, fix_scale):
    """NavState::IncSmall with USE_P_PLUS_RDP and SO3ex::exp's 1e-5 branch -> (state, theta < 1e-5)"""
    q = st[3:7]
    r = quat_rot(q, d[0:3])
    p = [st[i] + r[i] for i in range(3)]
    theta = mpmath.sqrt(d[3] * d[3] + d[4] * d[4] + d[5] * d[5])
    small = theta < EPS
    if small:
        t2 = theta * theta
        imag, real = HALF - t2 / 48, 1 - t2 / 8
    else:
        half = HALF * theta
        imag, real = mpmath.sin(half) / theta, mpmath.cos(half)
    e = quat_normalize([imag * d[3], imag * d[4], imag * d[5], real])
    q = quat_normalize(quat_mul(q, e))
    return p + q + [st[7] if fix_scale else st[7] + d[6]], small


def huber(e2, delta, dsqr):
    """RobustKernelHuber::robustify -> (rho[0], rho[1], inlier)"""
    if e2 <= dsqr:
        return [e2, mpf(1)], True
    sq = mpmath.sqrt(e2)
    return [2 * sq * delta - dsqr, delta / sq], False


def ldlt_solve(acc, lam, n):
    """(H + lambda I) x = b on the leading n x n block of the packed upper triangle, from its definition; the pivots of
    the LDL^T without pivoting are the ratios of the leading minors -> (x[7] with zeros behind n, or None where a pivot
    is not positive; the pivots)"""
    H = mpmath.zeros(n, n)
    k = 0
    for i in range(7):
        for j in range(i, 7):
            if j < n:
                H[i, j] = H[j, i] = acc[k]
            k += 1
    for i in range(n):
        H[i, i] += lam
    piv, prev = [], mpf(1)
    for m in range(1, n + 1):
        det = mpmath.det(H[0:m, 0:m])
        piv.append(det / prev)
        if not piv[-1] > 0:
            return None, piv
        prev = det
    x = mpmath.lu_solve(H, mpmath.matrix([acc[28 + i] for i in range(n)]))
    return [x[i] for i in range(n)] + [mpf(0)] * (7 - n), piv


# ---------------------------------------------------------------------------------------- OptimizeSim3's edges
# EdgeReproject<2, 6, 3, MODE> of src/Odom/g2otypes.h:321-549, MODE 1 (EdgeReprojectPRS) and MODE 2 (EdgeReprojectPRSInv),
# restated literally as the header restates them.  A camera is dict(ar = the camera of tests/algebra_ref.py, Rcb[9],
# tcb[3]); the image point is the float the camera model returns (Vec2data).
def _dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _edge_point(mode, cam, st, X):
    p, q, s = st[0:3], st[3:7], st[7]
    Rwb, Rcb, tcb = quat_to_mat(q), cam["Rcb"], cam["tcb"]
    scale = s
    if mode == 2:
        scale = 1 / scale
        twb = [-_dot3([Rwb[i], Rwb[3 + i], Rwb[6 + i]], p) for i in range(3)]
        Rcw = [_dot3(Rcb[3 * i:3 * i + 3], [Rwb[j], Rwb[3 + j], Rwb[6 + j]]) for i in range(3) for j in range(3)]
        tcw = [(-_dot3(Rcw[3 * i:3 * i + 3], twb) + tcb[i]) * scale for i in range(3)]
    else:
        Rcw = [_dot3(Rcb[3 * i:3 * i + 3], Rwb[3 * j:3 * j + 3]) for i in range(3) for j in range(3)]
        tcw = [-_dot3(Rcw[3 * i:3 * i + 3], p) + tcb[i] for i in range(3)]
    Xw = [x * scale for x in X]
    Pc = [_dot3(Rcw[3 * i:3 * i + 3], Xw) + tcw[i] for i in range(3)]
    return Rwb, Rcw, tcw, Xw, Pc, scale


def s3o_edge(mode, cam, st, X, obs):
    """-> (e[2], J[14] row-major 2 x 7: dP, dPhi, ds, info): info = dict(margin: how close the unrounded image point is to
    a point where its float changes, Pc, kb8: the camera model's branch, ds_terms: per row the sum of the absolute values of
    the products that make up the ds entry)"""
    from tests import algebra_ref as AR
    p = st[0:3]
    Rcb = cam["Rcb"]
    Rwb, Rcw, tcw, Xw, Pc, scale = _edge_point(mode, cam, st, X)
    uv, Jp = AR.cam_project_aw(cam["ar"], Pc)
    raw, _ = AR.cam_project_aw(cam["ar"], Pc, rounded=False)
    e = [obs[0] - uv[0], obs[1] - uv[1]]
    Jp = [-v for v in Jp]
    J, ds_terms = [], []
    for r in range(2):
        jp = Jp[3 * r:3 * r + 3]
        A = [_dot3(jp, [-Rcb[j], -Rcb[3 + j], -Rcb[6 + j]]) for j in range(3)]
        J0 = [_dot3(jp, [Rcw[j], Rcw[3 + j], Rcw[6 + j]]) for j in range(3)]
        if mode == 2:
            M = [_dot3(jp, [-Rcw[j], -Rcw[3 + j], -Rcw[6 + j]]) for j in range(3)]
            v = Xw
            dP = [_dot3(A, [-Rwb[j], -Rwb[3 + j], -Rwb[6 + j]]) for j in range(3)]
        else:
            M = [_dot3(jp, [Rcb[j], Rcb[3 + j], Rcb[6 + j]]) for j in range(3)]
            d = [Xw[i] - p[i] for i in range(3)]
            v = [_dot3([Rwb[j], Rwb[3 + j], Rwb[6 + j]], d) for j in range(3)]
            dP = A
        dPhi = [M[1] * v[2] - M[2] * v[1], -M[0] * v[2] + M[2] * v[0], M[0] * v[1] - M[1] * v[0]]
        js = _dot3(J0, X)
        terms = sum(abs(J0[i] * X[i]) for i in range(3))
        if mode == 2:
            js = (js + _dot3(jp, tcw)) * (-scale * scale)
            terms = (terms + sum(abs(jp[i] * tcw[i]) for i in range(3))) * scale * scale
        ds_terms.append(terms)
        J += dP + dPhi + [js]
    branch = AR.kb8_project_branch(cam["ar"], Pc) if cam["ar"]["model"] == 2 else "-"
    return e, J, dict(margin=min(AR.f32_margin(t) for t in raw), Pc=Pc, kb8=branch, ds_terms=ds_terms)


def s3o_edge_exact(mode, cam, st, X, obs):
    """the unrounded error obs - project(Pc) of the camera model itself"""
    from tests import algebra_ref as AR
    Pc = _edge_point(mode, cam, st, X)[4]
    uv = AR.cam_project_ex(cam["ar"], Pc)
    return [obs[0] - uv[0], obs[1] - uv[1]]


def s3o_edge_J_by_differences(mode, cam, st, X, obs, h=mpf(10) ** -20):
    """d e / d (dp, dphi, ds) by central differences of the unrounded error through the retraction s3o_inc_small"""
    J = [None] * 14
    for k in range(7):
        d = [mpf(0)] * 7
        d[k] = h
        ep = s3o_edge_exact(mode, cam, inc_small(st, d, False)[0], X, obs)
        d[k] = -h
        em = s3o_edge_exact(mode, cam, inc_small(st, d, False)[0], X, obs)
        J[k], J[7 + k] = (ep[0] - em[0]) / (2 * h), (ep[1] - em[1]) / (2 * h)
    return J


def s3o_chi2(e, info):
    return e[0] * (info * e[0]) + e[1] * (info * e[1])


def s3o_add_edge(e, J, info, delta, dsqr):
    """BaseMultiEdge::constructQuadraticForm of one edge into zeroed accumulators -> (acc[36] + [chi2], inlier)"""
    chi2 = s3o_chi2(e, info)
    (r0, r1), inlier = huber(chi2, delta, dsqr)
    w = r1 * info
    o0, o1 = -(info * e[0]) * r1, -(info * e[1]) * r1
    H, b = [], []
    for i in range(7):
        a0, a1 = J[i] * w, J[7 + i] * w
        H += [a0 * J[j] + a1 * J[7 + j] for j in range(i, 7)]
        b.append(J[i] * o0 + J[7 + i] * o1)
    return H + b + [r0, chi2], inlier


# ---------------------------------------------------------------------------------------- exact definitions
def exp_exact(u):
    """(sR [9], t [3], s): exp of the generator [[sigma I + Omega, upsilon], [0, 0]] by its series, 50 digits"""
    G = mpmath.zeros(4, 4)
    O = _skew(u[0:3])
    for i in range(3):
        for j in range(3):
            G[i, j] = O[3 * i + j] + (u[6] if i == j else 0)
        G[i, 3] = u[3 + i]
    # scale and square: the series converges fast below norm 1/2
    nrm = max(sum(abs(G[i, j]) for j in range(4)) for i in range(4))
    k = 0
    while nrm > mpf(1) / 2:
        nrm, k = nrm / 2, k + 1
    Gs = G / (2 ** k)
    E, term = mpmath.eye(4), mpmath.eye(4)
    for n in range(1, 80):
        term = term * Gs / n
        E = E + term
        if max(abs(x) for x in term) < mpf(10) ** -60:
            break
    for _ in range(k):
        E = E * E
    return [E[i, j] for i in range(3) for j in range(3)], [E[i, 3] for i in range(3)], mpmath.exp(u[6])
