"""Python restatement of the first half of LoopClosing::ComputeSim3 of the reference, the yardstick of
tests/test_loop_sim3.py: ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*) (src/ORBmatcher.cc:726-905) and Sim3Solver
(src/Sim3Solver.cc: SetRansacParameters, iterate, ComputeSim3, CheckInliers, Project).  Plain numpy, float64, one
statement of the reference per statement here; the eigenvector of Horn's N comes from LAPACK (eigh), which is the
independent solver the device's Jacobi is compared with.  The float steps of CheckInliers (crP3D, the image point, the
squared distance, the integer thresholds) are the reference's; Horn's closed form is in float64 where the reference
computes in CV_32F."""
import bisect
import math

import numpy as np

from tests.reloc_ref import HISTO_LENGTH, TH_LOW, descriptor_distance, three_maxima

f32 = np.float32
f64 = np.float64


# ---------------------------------------------------------------------------------------------------------------------
# ComputeSim3 (:220-322)
def horn_n_matrix(P1, P2):
    """Steps 1-3 on the 3 pairs P1[i] / P2[i]: (N, O1, O2, Pr1, Pr2)"""
    P1, P2 = np.asarray(P1, f64), np.asarray(P2, f64)
    O1, O2 = P1.sum(axis=0) / 3, P2.sum(axis=0) / 3
    Pr1, Pr2 = P1 - O1, P2 - O2
    M = Pr2.T @ Pr1  # Pr2 * Pr1^T of the reference's 3 x N matrices
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                  [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                  [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                  [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
    N = N + np.triu(N, 1).T
    return N, O1, O2, Pr1, Pr2


def rodrigues(r):
    """cv::Rodrigues, vector -> matrix"""
    theta = float(np.linalg.norm(r))
    if theta < np.finfo(f64).eps:
        return np.eye(3)
    c, s = math.cos(theta), math.sin(theta)
    x, y, z = np.asarray(r, f64) / theta
    return c * np.eye(3) + (1 - c) * np.outer([x, y, z], [x, y, z]) + s * np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])


def horn_sim3(P1, P2, fix_scale):
    """(R12, t12, s12, gap): Horn's closed form on 3 pairs; gap = the distance of N's two largest eigenvalues relative to
    the largest magnitude (the conditioning of the eigenvector)"""
    N, O1, O2, Pr1, Pr2 = horn_n_matrix(P1, P2)
    w, V = np.linalg.eigh(N)  # ascending
    q = V[:, 3]               # evec.row(0) of cv::eigen: the largest eigenvalue
    vec = q[1:]
    nv = float(np.linalg.norm(vec))
    ang = math.atan2(nv, q[0])
    R = rodrigues(2 * ang * vec / nv) if nv > 0 else np.eye(3)
    P3 = Pr2 @ R.T
    if not fix_scale:
        s = float((Pr1 * P3).sum() / (P3 * P3).sum())
    else:
        s = 1.0
    t = O1 - s * (R @ O2)
    scale = max(abs(w[0]), abs(w[3]))
    return R, t, s, float((w[3] - w[2]) / scale) if scale > 0 else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# Project (:352-373), CheckInliers (:324-344)
def cam_project(cam, Pc):
    """camm::{Pinhole,Radtan,KB8}Camera::Project on points Pc (n, 3) of one camera record: the float image points"""
    x, y, z = Pc[:, 0], Pc[:, 1], Pc[:, 2]
    fx, fy, cx, cy = (float(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    d = cam["dist"].astype(f64)
    with np.errstate(all="ignore"):
        invz = 1.0 / z
        pin = np.stack([fx * x * invz + cx, fy * y * invz + cy], axis=1)
        if cam["model"] == 1:
            nk = int(cam["num_k"])
            xn, yn = x * invz, y * invz
            x2, y2, xy = xn * xn, yn * yn, xn * yn
            r2 = x2 + y2
            fd, term = np.ones_like(r2), np.ones_like(r2)
            for i in range(nk):
                term = term * r2
                fd = fd + d[i] * term
            p1, p2 = d[nk], d[nk + 1]
            xd = xn * fd + 2 * p1 * xy + p2 * (r2 + 2 * x2)
            yd = yn * fd + 2 * p2 * xy + p1 * (r2 + 2 * y2)
            out = np.stack([fx * xd + cx, fy * yd + cy], axis=1)
        elif cam["model"] == 2:
            r = np.sqrt(x * x + y * y)
            th = np.arctan2(r, z)
            t2 = th * th
            thd = th * (1 + t2 * (d[0] + t2 * (d[1] + t2 * (d[2] + t2 * d[3]))))
            out = np.where((r > float(f32(1e-5)))[:, None], np.stack([fx * (x * thd / r) + cx, fy * (y * thd / r) + cy], axis=1), pin)
        else:
            out = pin
    return out.astype(f32)


def project(X, cams, cam_idx, A=None, t=None):
    """Project: crP3D = X, or A X + t rounded to float; the camera's Tcr (Rcb / tcb of the record); the model"""
    P = np.asarray(X, f32).astype(f64)
    if A is not None:
        with np.errstate(all="ignore"):
            P = np.stack([A[r, 0] * P[:, 0] + A[r, 1] * P[:, 1] + A[r, 2] * P[:, 2] + t[r] for r in range(3)], axis=1)
            P = P.astype(f32).astype(f64)
    out = np.zeros((len(P), 2), f32)
    for c in range(len(cams)):
        sel = np.flatnonzero(np.asarray(cam_idx) == c)
        if not len(sel):
            continue
        Rc, tc = cams[c]["Rcb"].reshape(3, 3), cams[c]["tcb"]
        Q = P[sel]
        Pc = np.stack([Rc[r, 0] * Q[:, 0] + Rc[r, 1] * Q[:, 1] + Rc[r, 2] * Q[:, 2] + tc[r] for r in range(3)], axis=1)
        out[sel] = cam_project(cams[c], Pc)
    return out


def _dist2(a, b):
    """dist.dot(dist) assigned to a float: float differences, the squares summed in double"""
    d = (a - b).astype(f64)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(f32)


def sim3_errors(R, t, s, c):
    """(err1, err2) of every correspondence of candidate c at the hypothesis (R, t, s), as CheckInliers compares them"""
    R, t, s = np.asarray(R, f64), np.asarray(t, f64), float(s)
    with np.errstate(all="ignore"):
        A12 = s * R
        A21 = (1.0 / s) * R.T
        t21 = np.array([-(A21[r, 0] * t[0] + A21[r, 1] * t[1] + A21[r, 2] * t[2]) for r in range(3)])
        p1im1, p2im2 = project(c["X1"], c["cams1"], c["cam1"]), project(c["X2"], c["cams2"], c["cam2"])
        p2im1 = project(c["X2"], c["cams1"], c["cam1"], A12, t)
        p1im2 = project(c["X1"], c["cams2"], c["cam2"], A21, t21)
        return _dist2(p1im1, p2im1), _dist2(p1im2, p2im2)


def check_inliers(R, t, s, c):
    err1, err2 = sim3_errors(R, t, s, c)
    with np.errstate(all="ignore"):
        return (err1 < np.asarray(c["max_err1"]).astype(f32)) & (err2 < np.asarray(c["max_err2"]).astype(f32))


# ---------------------------------------------------------------------------------------------------------------------
# SetRansacParameters (:118-141)
def ransac_parameters(N, probability=0.99, min_inliers=6, max_iterations=300):
    """(mRansacMinInliers, mRansacMaxIts).  N < minInliers: the solver never iterates (bNoMore at :148) and the
    reference's count is a NaN converted to int; reported as 1."""
    if N < min_inliers:
        return min_inliers, 1
    eps = f32(min_inliers) / f32(N)
    if min_inliers == N:
        its = 1
    else:
        its = int(math.ceil(math.log(1 - probability) / math.log(1 - float(eps) ** 3)))
    return min_inliers, max(1, min(its, max_iterations))


def t12_float(R, t, s):
    T = np.eye(4, dtype=f32)
    T[:3, :3] = (float(s) * np.asarray(R, f64)).astype(f32)
    T[:3, 3] = np.asarray(t, f64).astype(f32)
    return T


class Sim3Result:
    def __init__(self, T12, no_more, inliers, n_inliers, row):
        self.T12, self.no_more, self.inliers, self.n_inliers, self.row = T12, no_more, inliers, n_inliers, row

    @property
    def found(self):
        return self.T12 is not None


class Sim3SolverRef:
    """Sim3Solver with its draws replaced by a table of sample rows (samples[S][3]).  tables = (sRt (S, 13), mask (S, n)
    bool): the hypotheses are looked up instead of computed (the replay of a device table)."""

    def __init__(self, cand, samples, params=None, horn=horn_sim3, tables=None):
        self.c, self.horn, self.tables = cand, horn, tables
        self.samples = np.asarray(samples, np.int64).reshape(-1, 3)
        self.N, self.n1 = len(cand["X1"]), int(cand["n1"])
        p = dict(probability=0.99, min_inliers=6, max_iterations=300)
        p.update(params or {})
        self.min_inliers, self.max_its = ransac_parameters(self.N, **p)
        self.iterations, self.best_inliers, self.best_row, self.best = 0, 0, -1, None

    def _row(self, row):
        if self.tables is not None:
            o, mask = self.tables[0][row], self.tables[1][row]
            return o[:9].reshape(3, 3), o[9:12], o[12], mask
        idx = self.samples[row]
        R, t, s = self.horn(self.c["X1"][idx].astype(f64), self.c["X2"][idx].astype(f64), self.c["fix_scale"])[:3]
        return R, t, s, check_inliers(R, t, s, self.c)

    def iterate(self, n_iterations):
        vb = np.zeros(self.n1, bool)
        if self.N < self.min_inliers:
            return Sim3Result(None, True, vb, 0, -1)
        current = 0
        while self.iterations < self.max_its and current < n_iterations:
            row = self.iterations
            if row >= len(self.samples):  # the table of draws is used up (the library: VIEO_E_CAPACITY)
                return Sim3Result(None, 2, vb, 0, -1)
            current += 1
            self.iterations += 1
            R, t, s, mask = self._row(row)
            n = int(mask.sum())
            if n >= self.best_inliers:
                self.best_inliers, self.best_row, self.best = n, row, (R, t, s)
                if n > self.min_inliers:
                    vb[np.asarray(self.c["index1"])[mask]] = True
                    return Sim3Result(t12_float(R, t, s), False, vb, n, row)
        return Sim3Result(None, self.iterations >= self.max_its, vb, 0, -1)

    def find(self):
        return self.iterate(self.max_its)

    def estimate(self):
        if self.best is None:
            return None
        R, t, s = self.best
        return np.asarray(R, f64).astype(f32), np.asarray(t, f64).astype(f32), f32(s)


def sim3_error(R, t, s, R0, t0, s0):
    """(|t - t0|, |Log(R0^T R)|, |s / s0 - 1|)"""
    from tests.reloc_ref import pose_error
    dt, dR = pose_error(R, t, R0, t0)
    return dt, dR, abs(float(s) / float(s0) - 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vpMatches12) (src/ORBmatcher.cc:726-905)
def _bow_kf_walk(kf1, kf2, node_pairs, dist, nn_ratio, check_orientation):
    """The body of the reference's while loop over the shared nodes, and the orientation filter.  node_pairs: the
    (indices of kf1, indices of kf2) of every shared node, ascending; dist(i1, i2): the Hamming distance."""
    match12 = np.full(len(kf1.keys), -1, np.int64)  # vpMatches12 as the key of kf2 that holds the map point
    matched2 = np.zeros(len(kf2.keys), bool)
    nmatches = 0
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    rot_erase = [[] for _ in range(HISTO_LENGTH)]
    held = {}  # mapmpcami2distkp12idhist; std::map::emplace leaves an existing entry as it is
    ev = dict(skipped=0, no_point=0, ratio=0, replaced=0, kept=0, rotation=0)
    factor = f32(1.0) / f32(HISTO_LENGTH)
    for idx1_list, idx2_list in node_pairs:
        for idx1 in idx1_list:
            mp1 = int(kf1.mp_id[idx1])
            if mp1 < 0:
                continue
            best1, best2, best_idx2 = 256, 256, -1
            for idx2 in idx2_list:
                if matched2[idx2]:
                    ev["skipped"] += 1
                    continue
                if kf2.mp_id[idx2] < 0:
                    ev["no_point"] += 1
                    continue
                d = dist(idx1, idx2)
                if d < best1:
                    best2, best1, best_idx2 = best1, d, idx2
                elif d < best2:
                    best2 = d
            if not best1 < TH_LOW:
                continue
            if not (f32(best1) < f32(nn_ratio) * f32(best2)):
                ev["ratio"] += 1
                continue
            if mp1 in held:
                old = held[mp1]
                if old[0] <= best1:
                    ev["kept"] += 1
                    continue
                ev["replaced"] += 1
                match12[old[1]] = -1
                matched2[old[2]] = False
                nmatches -= 1
                if check_orientation:
                    rot_erase[old[3]].append(old[4])
            match12[idx1] = best_idx2
            matched2[best_idx2] = True
            entry = (best1, idx1, best_idx2, -1, -1)
            if check_orientation:
                rot = f32(kf1.keys["angle"][idx1]) - f32(kf2.keys["angle"][best_idx2])
                if rot < 0.0:
                    rot = f32(rot + f32(360.0))
                b = int(math.floor(float(f32(rot * factor)) + 0.5))
                if b == HISTO_LENGTH:
                    b = 0
                assert 0 <= b < HISTO_LENGTH
                entry = (best1, idx1, best_idx2, b, len(rot_hist[b]))
                rot_hist[b].append(idx1)
            held.setdefault(mp1, entry)
            nmatches += 1
    if check_orientation:
        hist2 = []
        for b in range(HISTO_LENGTH):
            h = list(rot_hist[b])
            for j in rot_erase[b]:
                h[j] = -1
            hist2.append([v for v in h if v != -1])
        keep = three_maxima([len(h) for h in hist2])
        for b in range(HISTO_LENGTH):
            if b in keep:
                continue
            for v in hist2[b]:
                match12[v] = -1
                nmatches -= 1
                ev["rotation"] += 1
    return match12.astype(np.int32), nmatches, ev


def search_by_bow_kf(kf1, kf2, nn_ratio, check_orientation):
    """The restatement: the two FeatureVectors are walked as the reference walks its two std::maps (equal ids: the
    node's body; otherwise lower_bound on the side that is behind), distances computed as they are needed.
    kf1 / kf2: objects with keys (angle), desc (n, 32) uint8, feat_vec [(node id, [indices])] ascending, mp_id."""
    A, B = kf1.feat_vec, kf2.feat_vec
    ids_a, ids_b = [n for n, _ in A], [n for n, _ in B]
    pairs, ia, ib = [], 0, 0
    while ia < len(A) and ib < len(B):
        if ids_a[ia] == ids_b[ib]:
            pairs.append((A[ia][1], B[ib][1]))
            ia, ib = ia + 1, ib + 1
        elif ids_a[ia] < ids_b[ib]:
            ia = bisect.bisect_left(ids_a, ids_b[ib])
        else:
            ib = bisect.bisect_left(ids_b, ids_a[ia])
    return _bow_kf_walk(kf1, kf2, pairs, lambda i, j: descriptor_distance(kf1.desc[i], kf2.desc[j]), nn_ratio,
                        check_orientation)


def search_by_bow_kf_brute(kf1, kf2, nn_ratio, check_orientation):
    """The brute-force statement: all n1 x n2 distances at once, the shared nodes from a set intersection."""
    bits_a, bits_b = np.unpackbits(kf1.desc, axis=1).astype(np.int32), np.unpackbits(kf2.desc, axis=1).astype(np.int32)
    D = bits_a @ (1 - bits_b).T + (1 - bits_a) @ bits_b.T
    A, B = dict(kf1.feat_vec), dict(kf2.feat_vec)
    pairs = [(A[n], B[n]) for n in sorted(set(A) & set(B))]
    return _bow_kf_walk(kf1, kf2, pairs, lambda i, j: int(D[i, j]), nn_ratio, check_orientation)
