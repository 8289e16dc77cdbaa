"""numpy restatement of the two projection searches of a loop closure that take a Sim3 world pose -- ORBmatcher::
SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th) (reference src/ORBmatcher.cc:507-626) and ORBmatcher::Fuse(
KeyFrame*, Scw, vpPoints, th, vpReplacePoint) (:1167-1220) -- on vieo_slam_amd.loop_closing.LoopKeyFrame objects and a
table of loop points (FUSE_POINT_DTYPE + ids).  Test infrastructure only.  Float expressions as in loop_verify_ref: numpy
float32 scalars in the reference's association order, 3 x 3 products row times column summed left to right."""
import math
from types import SimpleNamespace

import numpy as np

from tests.loop_verify_ref import F, GRID_COLS, GRID_ROWS, INT_MAX, build_grid, cam_project, mat3_vec, project_stage

TH_LOW = 50


def decompose_eigen(Scw):
    """:510-515: (Rcrw, tcrw, twcr) in Eigen float"""
    S = np.asarray(Scw, F).reshape(3, 4)
    scw = np.sqrt((S[0, 0] * S[0, 0] + S[0, 1] * S[0, 1]) + S[0, 2] * S[0, 2])
    R = (S[:, :3] / scw).astype(F)
    t = (S[:, 3] / scw).astype(F)
    return R, t, -mat3_vec(R.T, t)


def decompose_cv(Scw):
    """:1170-1173 with OpenCV's arithmetic as include/vieo_hot.h assumes it: Mat::dot and sqrt in double, scw rounded to
    float, Mat / scalar as the product with the double reciprocal rounded to float"""
    S = np.asarray(Scw, F).reshape(3, 4)
    dot = (float(S[0, 0]) * float(S[0, 0]) + float(S[0, 1]) * float(S[0, 1])) + float(S[0, 2]) * float(S[0, 2])
    scw = F(math.sqrt(dot))
    inv = 1.0 / float(scw)
    R = np.array([[F(float(S[r, c]) * inv) for c in range(3)] for r in range(3)], F)
    return R, np.array([F(float(S[r, 3]) * inv) for r in range(3)], F)


# ---------------------------------------------------------------------------------------------------------------------
# SearchByProjection(KeyFrame*, Scw, ...)
def _window(kf, grids, c, u, v, radius):
    """FrameBase::GetFeaturesInArea (FrameBase.cpp:95-141): [(position in the walk over all keys of the window's cells,
    key)] of the keys inside the square, cell columns ascending, rows ascending, a cell's keys ascending"""
    b = kf.bounds[c]
    winv, hinv = F(GRID_COLS) / (b[1] - b[0]), F(GRID_ROWS) / (b[3] - b[2])
    x0 = max(0, int(np.floor((u - b[0] - radius) * winv)))
    x1 = min(GRID_COLS - 1, int(np.ceil((u - b[0] + radius) * winv)))
    y0 = max(0, int(np.floor((v - b[2] - radius) * hinv)))
    y1 = min(GRID_ROWS - 1, int(np.ceil((v - b[2] + radius) * hinv)))
    if x0 >= GRID_COLS or x1 < 0 or y0 >= GRID_ROWS or y1 < 0:
        return []
    out, pos = [], 0
    for ix in range(x0, x1 + 1):
        for iy in range(y0, y1 + 1):
            for k in grids[c].get((ix, iy), ()):
                kp = kf.keys[k]
                if abs(kp["x"] - u) < radius and abs(kp["y"] - v) < radius:
                    out.append((pos, k))
                pos += 1
    return out


def _project(kf, R, t, twcr, P, c, th, cone=True):
    """:538-580 for camera c: (u, v, predicted level, radius) or None"""
    X, Pn = P["Xw"], P["normal"]
    Pcr = mat3_vec(R, X) + t
    Tc = kf.Tcr[c].reshape(3, 4)
    Pc = np.array([((Tc[r, 0] * Pcr[0] + Tc[r, 1] * Pcr[1]) + Tc[r, 2] * Pcr[2]) + Tc[r, 3] for r in range(3)], F)
    trc = kf.trc[c]
    twc = np.array([twcr[r] + ((R[0, r] * trc[0] + R[1, r] * trc[1]) + R[2, r] * trc[2]) for r in range(3)], F)
    if Pc[2] <= 0:
        return None
    invz = F(1) / Pc[2]
    cam = kf.cams[c]
    if not kf.use_distort:
        p0, p1 = Pc[0] * invz, Pc[1] * invz
        u = (cam["fx"] * p0 + F(0) * p1) + cam["cx"] * F(1)
        v = (F(0) * p0 + cam["fy"] * p1) + cam["cy"] * F(1)
    else:
        u, v = cam_project(cam, Pc)
    b = kf.bounds[c]
    if not (b[0] <= u < b[1] and b[2] <= v < b[3]):
        return None
    PO = X - twc
    dist = np.sqrt((PO[0] * PO[0] + PO[1] * PO[1]) + PO[2] * PO[2])
    if dist < F(0.8) * P["min_distance"] or dist > F(1.2) * P["max_distance"]:
        return None
    if cone and float((PO[0] * Pn[0] + PO[1] * Pn[1]) + PO[2] * Pn[2]) < 0.5 * float(dist):
        return None
    ratio = P["max_distance"] / dist
    lvl = int(np.ceil(F(np.log(np.float64(ratio))) / kf.log_scale_factor))
    lvl = min(max(lvl, 0), kf.n_levels - 1)
    return u, v, lvl, F(th) * kf.scale_factors[lvl]


def _hamming(a, b):
    return int(np.unpackbits(a ^ b).sum())


def search_by_projection_scw(kf, Scw, points, ids, matched, th=10.0, cone=True):
    """int ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) with the reference's structure: vpMatched is
    consulted inside the candidate loop.  returns (matched after the call, nmatches)."""
    R, t, twcr = decompose_eigen(Scw)
    matched = np.array(matched, np.int32)
    already = set(int(i) for i in matched if i >= 0)
    grids = [build_grid(kf, c) for c in range(kf.n_cams)]
    nmatches = 0
    for iMP in range(len(points)):
        P = points[iMP]
        if int(P["skip_mask"]) < 0 or int(ids[iMP]) in already:
            continue
        for cami in range(kf.n_cams):
            g = _project(kf, R, t, twcr, P, cami, th, cone)
            if g is None:
                continue
            u, v, lvl, radius = g
            bestDist, bestIdx = 256, -1
            for _, idx in _window(kf, grids, cami, u, v, radius):
                if matched[idx] >= 0:
                    continue
                kpLevel = int(kf.keys[idx]["octave"])
                if kpLevel < lvl - 1 or kpLevel > lvl:
                    continue
                dist = _hamming(P["desc"], kf.desc[idx])
                if dist < bestDist:
                    bestDist, bestIdx = dist, idx
            if bestDist <= TH_LOW:
                matched[bestIdx] = ids[iMP]
                nmatches += 1
    return matched, nmatches


def scw_lists(kf, Scw, points, ids, matched, th=10.0, cone=True):
    """what the device stage lists: per point, per camera, every window key of the predicted levels with Hamming distance
    <= TH_LOW as (key, distance, position in the walk), in the walk's order; [] for a point that is not searched"""
    R, t, twcr = decompose_eigen(Scw)
    already = set(int(i) for i in matched if i >= 0)
    grids = [build_grid(kf, c) for c in range(kf.n_cams)]
    out = []
    for iMP in range(len(points)):
        P = points[iMP]
        per_cam = [[] for _ in range(kf.n_cams)]
        if not (int(P["skip_mask"]) < 0 or int(ids[iMP]) in already):
            for c in range(kf.n_cams):
                g = _project(kf, R, t, twcr, P, c, th, cone)
                if g is None:
                    continue
                u, v, lvl, radius = g
                for pos, k in _window(kf, grids, c, u, v, radius):
                    if lvl - 1 <= int(kf.keys[k]["octave"]) <= lvl:
                        d = _hamming(P["desc"], kf.desc[k])
                        if d <= TH_LOW:
                            per_cam[c].append((int(k), d, pos))
        out.append(per_cam)
    return out


def replay_lists(lists, ids, matched):
    """the second statement: the lists replayed in the reference's order -- per item the smallest distance among the keys
    still free, the earlier candidate on equal distance"""
    matched = np.array(matched, np.int32)
    n = 0
    for iMP, per_cam in enumerate(lists):
        for cands in per_cam:
            free = [(d, pos, k) for k, d, pos in cands if matched[k] < 0]
            if free:
                matched[min(free)[2]] = ids[iMP]
                n += 1
    return matched, n


# ---------------------------------------------------------------------------------------------------------------------
# Fuse(KeyFrame*, Scw, ...)
def fuse_mask(kf, ids):
    """vbAlreadyMatched1 as written at :1177-1187: the camera looked up is that of KEY index iMP (0 past the keys)"""
    found = set((int(m), int(c)) for m, c in zip(kf.mp_id, kf.cam_of_key) if m >= 0)  # GetMapPointsCami
    mask = np.zeros(len(ids), np.int64)
    for iMP in range(len(ids)):
        cami = 0 if len(kf.keys) <= iMP else int(kf.cam_of_key[iMP])
        if (int(ids[iMP]), cami) in found:
            mask[iMP] |= 1 << cami
    return mask


def fuse_source(points, ids):
    """the loop points as project_stage reads a source key frame: isBad() points hold no map point"""
    bad = points["skip_mask"] < 0
    return SimpleNamespace(keys=np.zeros(len(points)), mp_id=np.where(bad, -1, np.asarray(ids, np.int64)), points=points)


def fuse_scw(kf, Scw, points, ids, th=4.0, detail=False):
    """int ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint): dict(match_key, replace, added, n_fused)"""
    R, t = decompose_cv(Scw)
    mask = fuse_mask(kf, ids)
    best_idx, best_dist = project_stage(fuse_source(points, ids), kf, R, t, th, mask, check_viewing_angle=True)
    n, nc = len(points), kf.n_cams
    vnMatch = [set() for _ in range(n)]
    match_key = np.full((n, nc), -1, np.int32)
    for i1 in range(n):
        for cami in range(nc):
            if best_idx[i1, cami] >= 0 and best_dist[i1, cami] <= TH_LOW:  # :193-196 (MatchMultiCam, fuselater)
                vnMatch[i1].add(int(best_idx[i1, cami]))
                match_key[i1, cami] = best_idx[i1, cami]
    holds = {k: int(m) for k, m in enumerate(kf.mp_id) if m >= 0}  # pKF->GetMapPoint
    replace, added, nFused = np.full(n, -1, np.int32), np.zeros((n, nc), np.uint8), 0
    for iMP in range(n):
        for bestIdx in sorted(vnMatch[iMP]):
            if bestIdx in holds:
                replace[iMP] = holds[bestIdx]
            else:
                holds[bestIdx] = int(ids[iMP])  # pKF->AddMapPoint(pMP, bestIdx)
                added[iMP, int(kf.cam_of_key[bestIdx])] = 1
            nFused += 1
    out = dict(match_key=match_key, replace=replace, added=added, n_fused=nFused)
    if detail:
        out.update(best_idx=best_idx, best_dist=best_dist, mask=mask, sets=[sorted(s) for s in vnMatch], transform=(R, t))
    return out


def oracle_project_stage(oracle, kf, R, t, th, points, ids, mask):
    """the search of fuse_scw through the oracle's vo_fuse_search with check_viewing_angle = 1 (loop_verify_ref's
    oracle_project_stage with the viewing cone on)"""
    from vieo_slam_amd.map_point import FUSE_FRAME_DTYPE
    FF = np.zeros(1, FUSE_FRAME_DTYPE)
    f = FF[0]["base"]
    f["Rcrw"], f["tcrw"], f["Ow"] = np.asarray(R, F).reshape(-1), t, kf.Ow
    f["n_cams"], f["use_distort"], f["cams"] = kf.n_cams, kf.use_distort, kf.cams.ctypes.data
    f["Tcr"][:kf.n_cams], f["trc"][:kf.n_cams], f["bounds"][:kf.n_cams] = kf.Tcr, kf.trc, kf.bounds
    f["log_scale_factor"], f["n_levels"] = kf.log_scale_factor, kf.n_levels
    FF[0]["scale_factors"][:kf.n_levels] = kf.scale_factors
    FF[0]["inv_level_sigma2"][:kf.n_levels] = kf.inv_level_sigma2
    FF[0]["th_radius"], FF[0]["check_viewing_angle"] = th, 1
    per_cam = [np.flatnonzero(kf.cam_of_key == c) for c in range(kf.n_cams)]
    pts = points.copy()
    pts["skip_mask"] = np.where(points["skip_mask"] >= 0, np.asarray(mask, np.int64), -2 ** 31).astype(np.int32)
    bi, bd = oracle.fuse_search(FF, [kf.keys[k] for k in per_cam], [None] * kf.n_cams, [kf.desc[k] for k in per_cam], pts)
    bi = bi.copy()
    for c in range(kf.n_cams):
        hit = bi[:, c] >= 0
        bi[hit, c] = per_cam[c][bi[hit, c]]
    return bi, bd


# ---------------------------------------------------------------------------------------------------------------------
# LoopClosing::ComputeSim3 (src/LoopClosing.cc:308-444) up to bMatch, composed from the restatements of its parts
def sim3_candidate(kf1, kf2, match12, fix_scale):
    """Sim3Solver's constructor (Sim3Solver.cc:22-116) on two LoopKeyFrame, through loop_closing.sim3_correspondences"""
    from vieo_slam_amd import loop_closing as lc
    m = np.asarray(match12)
    matched = np.where(m >= 0, kf2.mp_id[np.maximum(m, 0)], -1)
    index_in_kf2, Pw = {}, {}
    for k, i in enumerate(kf2.mp_id):
        if i >= 0:
            index_in_kf2.setdefault(int(i), []).append(k)
            Pw.setdefault(int(i), kf2.points[k]["Xw"])
    for i1 in np.flatnonzero(m >= 0):  # GetWorldPos of the matched point is read from the matched key
        if matched[i1] >= 0:
            Pw[int(matched[i1])] = kf2.points[int(m[i1])]["Xw"]
    for k, i in enumerate(kf1.mp_id):
        if i >= 0:
            Pw[int(i)] = kf1.points[k]["Xw"]

    def T(kf):
        M = np.eye(4, dtype=np.float32)
        M[:3, :3], M[:3, 3] = kf.Rcw, kf.tcw
        return M

    def cams(kf):
        if not kf.use_distort:
            c = lc.pinhole_camera((kf.cams[0]["fx"], kf.cams[0]["fy"], kf.cams[0]["cx"], kf.cams[0]["cy"]))
            return c, None
        c = kf.cams.copy()
        for i in range(kf.n_cams):
            M = kf.Tcr[i].reshape(3, 4).astype(np.float64)
            c[i]["Rcb"], c[i]["tcb"] = M[:, :3].reshape(-1), M[:, 3]
        return c, kf.cam_of_key
    c1, k1 = cams(kf1)
    c2, k2 = cams(kf2)
    cand = lc.sim3_correspondences(kf1.mp_id, matched, index_in_kf2, Pw, T(kf1), T(kf2), kf1.keys["octave"], kf2.keys["octave"],
                                   kf1.level_sigma2, kf2.level_sigma2, k1, k2, c1, c2, fix_scale)
    # X = Rcw Xw + tcw in float, row times column summed left to right (sim3_correspondences leaves the order to numpy)
    for name, kf, key in (("X1", kf1, lambda i1: i1), ("X2", kf2, lambda i1: int(m[i1]))):
        cand[name] = np.array([mat3_vec(kf.Rcw, kf.points[key(int(i1))]["Xw"]) + kf.tcw for i1 in cand["index1"]], F).reshape(-1, 3)
    return cand


def compose_scw(S12, kf2):
    """mg2oScw = gScm * gSmw in double, the float mScw"""
    s, R12, t12 = float(S12[0]), np.asarray(S12[1], np.float64).reshape(3, 3), np.asarray(S12[2], np.float64)
    R2, t2 = kf2.Rcw.astype(np.float64), kf2.tcw.astype(np.float64)
    R, t = R12 @ R2, s * (R12 @ t2) + t12
    return s, R, t, np.concatenate([s * R, t[:, None]], axis=1).astype(F)


def compute_sim3(kf1, cands, thresh_matches, min_inliers, fix_scale, samples, tables=None, max_passes=1000):
    """returns dict(found, cand, n_inliers, S12, s, R, t, Scw, match12, trace, passes, candidates = the solver inputs).
    samples[c]: (S, 3) rows of candidate c; tables[c]: (sRt, mask) of a device table to replay instead of Horn in numpy."""
    from tests import loop_optimize_ref as oref
    from tests import loop_ref
    from tests import loop_verify_ref as vref
    trace, solvers, bow, inputs = [], {}, {}, {}
    for c, kf2 in enumerate(cands):
        m, n, _ = loop_ref.search_by_bow_kf(kf1.bow, kf2.bow, 0.75, True)
        if n < thresh_matches:
            trace.append((c, 0, -1, 1, 0, n, -1, -1))
            continue
        trace.append((c, 0, -1, 0, 0, n, -1, -1))
        bow[c] = np.asarray(m, np.int32)
        inputs[c] = sim3_candidate(kf1, kf2, bow[c], fix_scale)
        solvers[c] = loop_ref.Sim3SolverRef(inputs[c], samples[c], dict(probability=0.99, min_inliers=min_inliers, max_iterations=300),
                                            tables=None if tables is None else tables[c])
    out = dict(found=False, cand=-1, n_inliers=0, match12=np.full(len(kf1.keys), -1, np.int32), candidates=inputs, passes=0)
    live, calls = set(solvers), {c: 0 for c in solvers}
    while live and not out["found"] and out["passes"] < max_passes:
        out["passes"] += 1
        for c in sorted(live):
            calls[c] += 1
            r = solvers[c].iterate(5)
            if r.no_more:
                live.discard(c)
            if not r.found:
                trace.append((c, calls[c], -1, int(r.no_more), 0, 0, -1, -1))
                continue
            m = np.where(r.inliers, bow[c], -1).astype(np.int32)
            R, t, s = solvers[c].estimate()
            m, n_found = vref.search_by_sim3(kf1, cands[c], s, R, t, m, 7.5)
            m, S12, n_inl, _ = oref.optimize_sim3(kf1, cands[c], float(s), R.astype(np.float64), t.astype(np.float64), m, 10.0, fix_scale)
            trace.append((c, calls[c], int(r.row), int(r.no_more), 1, int(r.n_inliers), int(n_found), int(n_inl)))
            if n_inl >= 20:
                sc, Rw, tw, Scw = compose_scw(S12, cands[c])
                out.update(found=True, cand=c, n_inliers=int(n_inl), S12=S12, s=sc, R=Rw, t=tw, Scw=Scw, match12=np.asarray(m, np.int32))
                break
    out["trace"] = trace
    return out
