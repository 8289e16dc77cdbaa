"""Named inputs of tests/test_solver_algebra.py: the lane functions of pnp_device.h and sim3_solver_device.h at generic
values and at the edges of their branches.  Every list is deterministic (seeded); a case is a tuple whose first entry
is its name.  Float inputs are float32 arrays."""
import itertools
import math

import numpy as np

from tests import algebra_cases as AC
from vieo_slam_amd import relocalization as rl

f32 = np.float32
K_PNP = np.array(rl.CAMERA_K, f32)


def _rot(rng, angle=None):
    w = rng.standard_normal(3)
    w /= np.linalg.norm(w)
    return rl.rodrigues(w * (rng.uniform(0.1, 3.0) if angle is None else angle))


def _next(x, up=True):
    return float(np.nextafter(f32(x), f32(np.inf if up else -np.inf)))


# ---------------------------------------------------------------------------------------------------------------------
# pnp_lstsq6<NC>: (name, A (6, NC), b (6,), kind); kind: "full", ("zero", column) or "deficient"
def lstsq_cases(nc, seed=1101):
    rng = np.random.default_rng([seed, nc])
    out = []
    for k in range(24):
        scale = (1.0, 1e-3, 1e6)[k % 3]
        out.append(("generic-%d" % k, rng.standard_normal((6, nc)) * scale, rng.standard_normal(6) * scale, "full"))
    for sign in (1, -1):  # A[k][k] > 0: alpha = -|column|; A[k][k] <= 0: alpha = +|column|
        A = rng.standard_normal((6, nc))
        for k in range(nc):
            A[k, k] = sign * (abs(A[k, k]) + 0.5)
        out.append(("diagonal-%s" % ("positive" if sign > 0 else "negative"), A, rng.standard_normal(6), "full"))
    A = rng.standard_normal((6, nc))
    A[0, 0] = 0.0
    out.append(("pivot-zero", A, rng.standard_normal(6), "full"))
    for j in (0, 1, nc - 1):
        A = rng.standard_normal((6, nc))
        A[:, j] = 0.0
        out.append(("zero-column-%d" % j, A, rng.standard_normal(6), ("zero", j)))
    for sign in (1, -1):  # column 0 is its pivot alone: the reflection maps e0 to -+ e0
        A = rng.standard_normal((6, nc))
        A[1:, 0] = 0.0
        A[0, 0] = sign * 1.75
        out.append(("column-reduced-to-its-pivot-%s" % ("positive" if sign > 0 else "negative"), A, rng.standard_normal(6), "full"))
    A = rng.standard_normal((6, nc))
    A = np.triu(A[:nc]).tolist() + [[0.0] * nc] * (6 - nc)  # already triangular: every column is its pivot
    out.append(("upper-triangular", np.array(A), rng.standard_normal(6), "full"))
    A = rng.integers(-4, 5, (6, nc)).astype(np.float64)
    A[:, nc - 1] = 3 * A[:, 0]
    out.append(("proportional-columns", A, rng.standard_normal(6), "deficient"))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# pnp_rot: (name, a, b, g)
def rot_cases(seed=1102):
    rng = np.random.default_rng(seed)
    out = [("zeta-positive", 1.0, 2.0, 0.5), ("zeta-negative", 2.0, 1.0, 0.5), ("zeta-positive-g-negative", 2.0, 1.0, -0.5),
           ("zeta-negative-g-negative", 1.0, 2.0, -0.5), ("g-tiny-zeta-squared-overflows", 1.0, 2.0, 1e-200),
           ("g-tiny-negative", 1.0, 2.0, -1e-200), ("a-equals-b", 1.5, 1.5, 0.3), ("a-equals-b-g-negative", 1.5, 1.5, -0.3),
           ("zeta-huge-no-overflow", 1.0, 2.0, 1e-100), ("g-dominates", 1.0, 1.0 + 1e-12, 1e6)]
    for k in range(60):
        a, b = rng.standard_normal(2) * 10.0 ** rng.integers(-3, 4)
        out.append(("generic-%d" % k, float(a), float(b), float(rng.standard_normal() * 10.0 ** rng.integers(-6, 3))))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# pnp_eig3: (name, S (3, 3) symmetric, kind); kind "unique": d and U compared; "invariants": d, residual, orthonormality
def _sym(Q, w):
    S = Q @ np.diag(w) @ Q.T
    return 0.5 * (S + S.T)


def eig3_cases(seed=1103):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(20):
        out.append(("generic-%d" % k, _sym(_rot(rng), np.sort(rng.uniform(0.1, 10.0, 3))[::-1] * 10.0 ** (k % 3 - 1)), "unique"))
    for k in range(10):  # the scatter of n points, as choose_control_points builds it
        P = rng.standard_normal((6 + 3 * k, 3)) * [3.0, 1.0, 0.3]
        P = (P - P.mean(axis=0)) @ _rot(rng).T
        out.append(("scatter-%d" % k, P.T @ P, "unique"))
    for perm in itertools.permutations((3.0, 2.0, 1.0)):
        out.append(("diagonal-%d%d%d" % tuple(int(p) for p in perm), np.diag(perm), "unique"))
    out.append(("double-diagonal", np.diag([2.0, 1.0, 2.0]), "invariants"))
    out.append(("double-rotated", _sym(_rot(rng), [2.0, 2.0, 1.0]), "invariants"))
    out.append(("double-smallest-rotated", _sym(_rot(rng), [3.0, 1.0, 1.0]), "invariants"))
    out.append(("triple-diagonal", 2.0 * np.eye(3), "invariants"))
    cube = np.array(list(itertools.product((-1.0, 1.0), repeat=3)))
    out.append(("triple-cube-corners", cube.T @ cube, "invariants"))
    out.append(("triple-rotated", _sym(_rot(rng), [2.0, 2.0, 2.0]), "invariants"))
    S = np.diag([1.0, 2.0, 3.0])
    S[0, 1] = S[1, 0] = 1e-19
    out.append(("off-diagonal-below-ulp-01", S, "unique"))
    S = np.diag([3.0, 2.0, 1.0])
    S[0, 2] = S[2, 0] = -1e-19
    S[1, 2] = S[2, 1] = 0.25
    out.append(("off-diagonal-below-ulp-02", S, "unique"))
    for k in range(3):
        a, b = rng.standard_normal(3), rng.standard_normal(3)
        out.append(("rank-2-%d" % k, np.outer(a, a) + np.outer(b, b), "unique"))
    a = np.array([1.0, 2.0, 2.0])
    out.append(("rank-1", np.outer(a, a), "invariants"))
    # eigenvectors whose largest component is negative in the basis they are built from
    Q = np.array([[-0.8, 0.6, 0.0], [-0.6, -0.8, 0.0], [0.0, 0.0, -1.0]]).T
    out.append(("negative-largest-components", _sym(Q, [5.0, 2.0, 1.0]), "unique"))
    # (1, 1, 0) and (1, -1, 0): the two largest components tie in magnitude; with opposite signs the convention's
    # choice hangs on the last bit, so the vectors are compared as lines
    out.append(("components-tie", np.array([[2.0, 0.5, 0.0], [0.5, 2.0, 0.0], [0.0, 0.0, 1.0]]), "invariants"))
    out.append(("components-tie-last", np.array([[4.0, 0.0, 0.0], [0.0, 2.0, -0.5], [0.0, -0.5, 2.0]]), "invariants"))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# pnp_polar3: (name, B (3, 3), kind); kind "unique": R compared; "invariants": orthogonality and |det| only
RZ90 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


def column_swaps(lengths2):
    """the number of exchanges pnp_polar3's three compare-exchanges make on these squared column lengths"""
    n2, swaps = list(lengths2), 0
    for i, j in ((0, 1), (1, 2), (0, 1)):
        if n2[i] < n2[j]:
            n2[i], n2[j] = n2[j], n2[i]
            swaps += 1
    return swaps


def polar3_cases(seed=1104):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(24):
        P = _sym(_rot(rng), rng.uniform(0.2, 5.0, 3) * 10.0 ** (k % 3 - 1))
        out.append(("generic-%d" % k, _rot(rng) @ P, "unique"))
    for perm in itertools.permutations((1.0, 2.0, 3.0)):
        tag = "%d%d%d" % tuple(int(p) for p in perm)
        out.append(("orthogonal-columns-%s" % tag, RZ90 @ np.diag(perm), "unique"))          # exact: no sweep
        out.append(("column-lengths-%s" % tag, _rot(rng) @ _sym(_rot(rng), [1.0, 1.3, 1.7]) @ np.diag(perm), "unique"))
    U, Vt = _rot(rng), _rot(rng)
    out.append(("sigma3-1e-12", U @ np.diag([1.0, 0.5, 1e-12]) @ Vt, "unique"))
    out.append(("sigma3-1e-12-negative", U @ np.diag([1.0, 0.5, -1e-12]) @ Vt, "unique"))
    out.append(("rank-2-exact", np.array([[1.0, 4.0, 5.0], [2.0, 5.0, 7.0], [3.0, 6.0, 9.0]]), "invariants"))
    out.append(("rank-2-zero-column", np.array([[1.0, 0.0, 0.5], [0.0, 0.0, 2.0], [-1.0, 0.0, 0.25]]), "invariants"))
    for k in range(3):
        P = _sym(_rot(rng), rng.uniform(0.5, 3.0, 3))
        out.append(("reflection-%d" % k, -(_rot(rng) @ P), "unique"))
    out.append(("reflection-diagonal", np.diag([3.0, 2.0, -1.0]), "unique"))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# pnp_alphas: (name, c0 (3,), ci (3, 3), X (3,) float32); pnp_project: (name, K, R, t, X)
def alphas_cases(seed=1105):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(30):
        Q, ks = _rot(rng), rng.uniform(0.2, 3.0, 3)
        out.append(("generic-%d" % k, rng.standard_normal(3) * 3, (Q / ks).T, (rng.standard_normal(3) * 3).astype(f32)))
    Q, ks = _rot(rng), rng.uniform(0.2, 3.0, 3)
    ci = (Q / ks).T
    ci[2] = 0.0
    out.append(("planar-frame", rng.standard_normal(3), ci, (rng.standard_normal(3) * 3).astype(f32)))
    c0 = np.array([1.5, -2.25, 4.0])
    out.append(("point-at-the-centroid", c0, (Q / ks).T, c0.astype(f32)))
    out.append(("world-offset-1e4", np.array([1e4, -1e4, 1e4]) + rng.standard_normal(3), (Q / ks).T,
                (np.array([1e4, -1e4, 1e4]) + rng.standard_normal(3)).astype(f32)))
    return out


def _invz_boundary(depth, rel):
    """a depth whose reciprocal lies at (1 + rel) times the midpoint of two neighbouring floats"""
    f = f32(1.0 / depth)
    mid = 0.5 * (float(f) + float(np.nextafter(f, f32(np.inf))))
    return 1.0 / (mid * (1.0 + rel))


def project_cases(seed=1106):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(30):
        R, t = _rot(rng, rng.uniform(0, 0.5)), rng.standard_normal(3) * 0.3
        z = rng.uniform(1.5, 12.0)
        Pc = np.array([rng.uniform(-0.7, 0.7) * z, rng.uniform(-0.5, 0.5) * z, z])
        out.append(("generic-%d" % k, K_PNP, R, t, (R.T @ (Pc - t)).astype(f32)))
    X = np.array([0.5, 0.25, 0.0], f32)  # R = I and X[2] = 0: P[2] is t[2] exactly
    for name, z in (("depth-1.5", 1.5), ("depth-200", 200.0)):
        out.append((name, K_PNP, np.eye(3), np.array([0.1, -0.2, z]), X))
    for depth in (1.5, 7.3, 200.0):
        for rel in (1e-9, -1e-9):
            out.append(("invz-next-to-a-rounding-boundary/depth=%g/%+g" % (depth, rel), K_PNP, np.eye(3),
                        np.array([0.1, -0.2, _invz_boundary(depth, rel)]), X))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# pnp_check_inliers: (name, K, R (3, 3), t (3,), Xw (n, 3), uv (n, 2), max_err (n,), fill)
CHECK_N = (1, 63, 64, 65, 127, 128, 129)


def check_cases():
    out = []
    for n in CHECK_N:
        s = rl.make_pnp_scene(300 + n, n, 0.3, 2.0)  # 2 px of noise at th2 = 5.991: inliers and outliers alternate
        me = (s["sigma2"] * f32(5.991)).astype(f32)
        for fill in (0, 1):
            out.append(("n=%d/%s" % (n, "words-hold-ones" if fill else "words-hold-zeros"), K_PNP, s["R"], s["t"], s["Xw"],
                        s["uv"], me, fill))
    # R = I, t = 0, X = (0, 0, 1), cx = 320, cy = 240: ue = cx, ve = cy exactly; the pixel is (323, 244): error2 = 25
    Kx = np.array([K_PNP[0], K_PNP[1], 320.0, 240.0], f32)
    uv = np.array([[323.0, 244.0]] * 3, f32)
    out.append(("error-equal-to-the-threshold", Kx, np.eye(3), np.zeros(3), np.array([[0, 0, 1]] * 3, f32), uv,
                np.array([25.0, _next(25.0), _next(25.0, False)], f32), 1))
    s = rl.make_pnp_scene(300 + 129, 129, 0.3, 2.0)
    me = (s["sigma2"] * f32(5.991)).astype(f32)
    for name, R, t in (("nan-in-R", np.where(np.eye(3) > 0, np.nan, s["R"]), s["t"]), ("inf-in-t", s["R"], np.array([0, np.inf, 0])),
                       ("nan-in-t", s["R"], np.array([0, 0, np.nan]))):
        out.append(("non-finite-pose/%s" % name, K_PNP, R, t, s["Xw"], s["uv"], me, 1))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# pnp_epnp: (name, K, Xw (n, 3) float32, uv (n, 2) float32, idx (cnt,) int32, truth (R, t) or None)
def scene_from_points(Pc, R, t, noise=0.0, rng=None, offset=None):
    """map points at Pc in the camera of pose (R, t), their noise-free (or noisy) pixels; offset: the world's origin"""
    fx, fy, cx, cy = (float(k) for k in K_PNP)
    if offset is not None:
        t = t - R @ offset          # Xw = R^T (Pc - t) lies offset away
    Xw = ((Pc - t) @ R).astype(f32)
    uv = np.stack([cx + fx * Pc[:, 0] / Pc[:, 2], cy + fy * Pc[:, 1] / Pc[:, 2]], axis=1)
    if noise:
        uv = uv + rng.standard_normal(uv.shape) * noise
    return Xw, uv.astype(f32), (R, t)


def _cloud(rng, n):
    z = rng.uniform(1.5, 12.0, n)
    return np.stack([rng.uniform(-0.7, 0.7, n) * z, rng.uniform(-0.45, 0.45, n) * z, z], axis=1)


def _pose(rng):
    return rl.rodrigues(rng.standard_normal(3) * 0.15), rng.standard_normal(3) * 0.3


# make_pnp_scene(seed, n, 0.0, noise) scenes that enter the rarer branches of compute_pose, found by a search with the
# host build's taps (n = 6 ... 20, noise 0 ... 40 px, 150 ... 400 seeds each); x[0] < 0 needs 5 px of noise on 6 points.
# tests/test_solver_algebra.py asserts each branch from the 50-digit reference and from the evaluator's taps.
BRANCH_SEEDS = {
    "x0-negative-in-guess-1": (2174, 6, 5.0),
    "x0-negative-in-guess-2": (2177, 6, 5.0),
    "x0-negative-in-guess-3": (2040, 6, 5.0),
    "x2-of-the-wrong-sign-in-guess-2": (1001, 6, 0.5),
    "x2-of-the-wrong-sign-in-guess-3": (1000, 6, 0.5),   # also x[1] < 0 in guesses 2 and 3, and z0 < 0
    "det-negative": (1106, 6, 2.0),
    "guess-2-wins": (3256, 6, 5.0),                      # its error 7.7 px against 440 and 146
}


def epnp_cases(seed=1107):
    rng = np.random.default_rng(seed)
    out = []
    for n in (6, 7, 8, 20, 60):
        R, t = _pose(rng)
        Xw, uv, truth = scene_from_points(_cloud(rng, n), R, t)
        out.append(("generic-n=%d" % n, K_PNP, Xw, uv, np.arange(n, dtype=np.int32), truth))
    for n in (8, 20):
        R, t = _pose(rng)
        Xw, uv, truth = scene_from_points(_cloud(rng, n), R, t, 0.5, rng)
        out.append(("noisy-n=%d" % n, K_PNP, Xw, uv, np.arange(n, dtype=np.int32), None))
    R, t = _pose(rng)
    Xw, uv, truth = scene_from_points(_cloud(rng, 30), R, t)
    out.append(("idx-permutes-and-skips", K_PNP, Xw, uv, rng.permutation(30)[:12].astype(np.int32), truth))
    # planar scenes: points of the plane z = 4 in the world, the camera looking at it
    n = 12
    grid = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), np.full(n, 4.0)], axis=1)
    R, t = _pose(rng)
    Xw = grid.astype(f32)
    Pc = Xw.astype(np.float64) @ R.T + t
    fx, fy, cx, cy = (float(k) for k in K_PNP)
    uv = np.stack([cx + fx * Pc[:, 0] / Pc[:, 2], cy + fy * Pc[:, 1] / Pc[:, 2]], axis=1).astype(f32)
    out.append(("planar-axis-aligned", K_PNP, Xw, uv, np.arange(n, dtype=np.int32), (R, t)))
    tilt = rl.rodrigues(np.array([0.4, -0.3, 0.2]))
    Xw = ((grid - [0, 0, 4.0]) @ tilt.T + [0, 0, 4.0]).astype(f32)
    Pc = Xw.astype(np.float64) @ R.T + t
    uv = np.stack([cx + fx * Pc[:, 0] / Pc[:, 2], cy + fy * Pc[:, 1] / Pc[:, 2]], axis=1).astype(f32)
    out.append(("planar-tilted", K_PNP, Xw, uv, np.arange(n, dtype=np.int32), None))
    Xw = (grid + np.stack([np.zeros(n), np.zeros(n), rng.uniform(-1e-3, 1e-3, n)], axis=1)).astype(f32)
    Pc = Xw.astype(np.float64) @ R.T + t
    uv = np.stack([cx + fx * Pc[:, 0] / Pc[:, 2], cy + fy * Pc[:, 1] / Pc[:, 2]], axis=1).astype(f32)
    out.append(("near-planar-1mm", K_PNP, Xw, uv, np.arange(n, dtype=np.int32), None))
    cube = np.array(list(itertools.product((-1.0, 1.0), repeat=3))) + [0, 0, 5.0]
    Xw = cube.astype(f32)
    Pc = Xw.astype(np.float64) @ R.T + t
    uv = np.stack([cx + fx * Pc[:, 0] / Pc[:, 2], cy + fy * Pc[:, 1] / Pc[:, 2]], axis=1).astype(f32)
    out.append(("cube-corners", K_PNP, Xw, uv, np.arange(8, dtype=np.int32), None))
    for off in (1e2, 1e3, 1e4):
        R, t = _pose(rng)
        Xw, uv, truth = scene_from_points(_cloud(rng, 10), R, t, offset=np.array([off, -off, off]))
        out.append(("world-offset-%g" % off, K_PNP, Xw, uv, np.arange(10, dtype=np.int32), None))
    for name, (sd, n, noise) in BRANCH_SEEDS.items():
        s = rl.make_pnp_scene(sd, n, 0.0, noise)
        out.append((name, K_PNP, s["Xw"], s["uv"], np.arange(n, dtype=np.int32), None))
    return out


def epnp_small_cases(seed=1108):
    """n = 4 and n = 5: properties and lane independence only (What EPnP leaves open)"""
    rng = np.random.default_rng(seed)
    out = []
    for n in (4, 4, 5, 5):
        R, t = _pose(rng)
        Xw, uv, truth = scene_from_points(_cloud(rng, n), R, t)
        out.append(("small-n=%d-%d" % (n, len(out)), K_PNP, Xw, uv, np.arange(n, dtype=np.int32), truth))
    return out


FIXED = ("generic-n=6", "generic-n=20", "planar-axis-aligned", "noisy-n=8", "small-n=4-0")   # repeated in lanes 0, 7, 15


def epnp_jobs(names):
    """the order in which the cases run: every case once (whole workgroups of 16 different cases, padded from the
    start of the list), then for each fixed case three workgroups that hold it in lane 0, 7 and 15 among shifting
    neighbours, then a last workgroup of five live lanes.  Returns the case index of every job."""
    n = len(names)
    jobs = list(range(n))
    jobs += [k % n for k in range((-n) % 16)]
    fixed = [names.index(f) for f in FIXED]
    for k, f in enumerate(fixed):
        for w, lane in enumerate((0, 7, 15)):
            wg = [(5 * k + 3 * w + 7 * j + 1) % n for j in range(16)]
            wg[lane] = f
            jobs += wg
    jobs += fixed
    assert len(jobs) % 16 == len(FIXED)
    return jobs


# ---------------------------------------------------------------------------------------------------------------------
# s3s_top_eigenvector: (name, N (4, 4) symmetric, kind)
def _horn_n(P1, P2):
    from tests import loop_ref
    return loop_ref.horn_n_matrix(P1, P2)[0]


def top_cases(seed=1109):
    rng = np.random.default_rng(seed)
    out = []
    for p in range(4):
        d = [1.0, 2.0, 3.0]
        d.insert(p, 4.0)
        out.append(("diagonal-maximum-at-%d" % p, np.diag(d), "unique"))
    out.append(("tie-of-the-two-largest", np.diag([1.0, 5.0, 2.0, 5.0]), "invariants"))
    out.append(("tie-rotated", np.array([[5.0, 0, 0, 0], [0, 5.0, 0, 0], [0, 0, 1.5, 0.5], [0, 0, 0.5, 1.5]]), "invariants"))
    N = np.diag([1.0, 2.0, 3.0, 4.0])
    N[0, 1] = N[1, 0] = 1e-19
    N[2, 3] = N[3, 2] = 0.25
    out.append(("off-diagonal-below-ulp", N, "unique"))
    for name, P1, P2, fix, kind in horn_cases():
        if kind == "unique":
            out.append(("horn/" + name, _horn_n(P1, P2), "unique"))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# s3s_horn: (name, P1 (3, 3), P2 (3, 3), fix_scale, kind); a point per row; P1 = s R P2 + t
def _triple(rng):
    return rng.standard_normal((3, 3)) * [2.0, 1.5, 1.0] + [0, 0, 5.0]


def horn_cases(seed=1110):
    rng = np.random.default_rng(seed)
    out = []

    def moved(P2, R, t, s):
        return s * (P2 @ R.T) + t

    for k in range(24):
        P2, R, t, s = _triple(rng), _rot(rng), rng.standard_normal(3), rng.uniform(0.5, 2.0)
        P1 = moved(P2, R, t, s) + (rng.standard_normal((3, 3)) * 0.01 if k % 2 else 0.0)
        out.append(("generic-%d" % k, P1.astype(f32).astype(np.float64), P2.astype(f32).astype(np.float64), k % 4 == 3, "unique"))
    P2 = _triple(rng)
    out.append(("same-points", P2, P2.copy(), False, "identity"))
    out.append(("same-points-fixed-scale", P2, P2.copy(), True, "identity"))
    axis = np.array([1.0, 2.0, -2.0]) / 3
    for th in (1e-9, 3e-9, 1e-6):
        out.append(("rotation-%g-rad" % th, moved(P2, rl.rodrigues(axis * th), np.zeros(3), 1.0), P2, False, "unique"))
    out.append(("rotation-90-degrees", moved(P2, RZ90, np.array([0.5, -1.0, 0.25]), 1.0), P2, False, "unique"))
    for name, ax in (("x", (1.0, 0, 0)), ("y", (0, 1.0, 0)), ("z", (0, 0, 1.0)), ("111", (1.0, 1.0, 1.0))):
        a = np.array(ax) / np.linalg.norm(ax)
        R = 2 * np.outer(a, a) - np.eye(3)  # a half turn, exactly for the coordinate axes
        out.append(("half-turn-about-%s" % name, moved(P2, R, np.zeros(3), 1.0), P2, False, "unique"))
    for th in (3.3, 4.0, 5.5, 6.2):  # beyond a half turn
        out.append(("rotation-%g-rad" % th, moved(P2, rl.rodrigues(axis * th), rng.standard_normal(3), 1.0), P2, False, "unique"))
    for s in (0.5, 1.0, 2.0):
        R, t = _rot(rng), rng.standard_normal(3)
        for fix in (False, True):
            out.append(("scale-%g/%s" % (s, "fixed" if fix else "free"), moved(P2, R, t, s), P2, fix, "unique"))
    line = np.array([[0.0, 0, 0], [1.0, 2.0, 0.5], [3.0, 6.0, 1.5]]) + [0.5, 0.25, 4.0]
    out.append(("collinear-triples", moved(line, _rot(rng), rng.standard_normal(3), 1.5), line, False, "invariants"))
    out.append(("collinear-triples-fixed-scale", moved(line, _rot(rng), rng.standard_normal(3), 1.0), line, True, "invariants"))
    same = np.array([[1.0, 2.0, 3.0]] * 3)
    out.append(("coincident-points-in-set-2", _triple(rng), same, False, "no-scale"))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# s3s_pose: (name, R, t, s); s3s_project: (name, camera index, A or None, t, X); s3s_dist2: (name, a, b);
# s3s_is_inlier: built in the test from the reference's own errors
def sim3_cameras():
    """indices into algebra_cases.cameras(): a pinhole with Tcr = identity, Radtan, KB8, a pinhole behind a body transform"""
    names, cams, _ = AC.cameras()
    pick = [names.index("pinhole"), names.index("radtan0-k2"), names.index("kb8-0"), names.index("pinhole-body")]
    assert not cams[pick[0]]["tcb"].any() and cams[pick[3]]["tcb"].any()
    return pick


def pose_cases(seed=1111):
    rng = np.random.default_rng(seed)
    out = [("generic-%d" % k, _rot(rng), rng.standard_normal(3) * 2, float(rng.uniform(0.3, 3.0))) for k in range(20)]
    for s in (0.5, 1.0, 2.0):
        out.append(("scale-%g" % s, _rot(rng), rng.standard_normal(3), s))
    return out


def _float_boundary(x, rel):
    f = f32(x)
    mid = 0.5 * (float(f) + float(np.nextafter(f, f32(np.inf))))
    return mid * (1.0 + rel)


def sim3_project_cases(seed=1112):
    rng = np.random.default_rng(seed)
    out = []
    for ci in sim3_cameras():
        for k in range(8):
            z = rng.uniform(2.0, 8.0)
            X = np.array([rng.uniform(-0.4, 0.4) * z, rng.uniform(-0.3, 0.3) * z, z], f32)
            out.append(("camera-%d/point-itself-%d" % (ci, k), ci, None, None, X))
            s, R, t = rng.uniform(0.7, 1.4), _rot(rng, rng.uniform(0, 0.2)), rng.standard_normal(3) * 0.1
            out.append(("camera-%d/transformed-%d" % (ci, k), ci, s * R, t, X))
        for rel in (1e-9, -1e-9):  # A = I and X[0] = 0: crP3D[0] is t[0] itself, next to the middle of two floats
            X = np.array([0.0, 0.4, 3.0], f32)
            out.append(("camera-%d/crP3D-next-to-a-rounding-boundary/%+g" % (ci, rel), ci, np.eye(3),
                        np.array([_float_boundary(0.3, rel), 0.0, 0.0]), X))
    return out


def dist2_cases(seed=1113):
    rng = np.random.default_rng(seed)
    out = [("exact-3-4", np.array([10.0, 20.0], f32), np.array([7.0, 16.0], f32)),
           ("same-point", np.array([10.5, 20.25], f32), np.array([10.5, 20.25], f32))]
    for k in range(40):
        a = rng.uniform(0, 752, 2).astype(f32)
        out.append(("generic-%d" % k, a, (a + rng.standard_normal(2) * 10.0 ** rng.integers(-3, 2)).astype(f32)))
    return out


def inlier_pairs(seed=1114):
    """(name, camera 1, camera 2, R, t, s, X1, X2): X1 = s R X2 + t up to a few centimetres"""
    rng = np.random.default_rng(seed)
    out = []
    cams = sim3_cameras()
    for k in range(8):
        c1, c2 = cams[k % 4], cams[(k // 2) % 4]
        s, R, t = rng.uniform(0.7, 1.4), _rot(rng, rng.uniform(0, 0.2)), rng.standard_normal(3) * 0.1
        z = rng.uniform(2.0, 8.0)
        X2 = np.array([rng.uniform(-0.3, 0.3) * z, rng.uniform(-0.2, 0.2) * z, z])
        X1 = s * (R @ X2) + t + rng.standard_normal(3) * 0.02
        out.append(("pair-%d/cameras-%d-%d" % (k, c1, c2), c1, c2, R, t, float(s), X1.astype(f32), X2.astype(f32)))
    return out
