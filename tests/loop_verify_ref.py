"""numpy restatement of ORBmatcher::SearchBySim3 (reference src/ORBmatcher.cc:1222-1301) with the search of
SearchByProjectionBase (:26-227) it calls twice, on vieo_slam_amd.loop_closing.LoopKeyFrame objects.  Test infrastructure
only.  Float expressions are evaluated on numpy float32 scalars in the reference's association order, every 3 x 3 product
row times column summed left to right (OpenCV's own small-matrix kernel is not pinned); the distorted
cameras project in double and round to float as camm::*Camera::Project does; logf is taken as the correctly rounded
double logarithm (oracle/mappoint.cc)."""
import math

import numpy as np

F = np.float32
TH_HIGH = 100
GRID_COLS, GRID_ROWS = 64, 48  # FrameBase.h:224-225
INT_MAX = 2 ** 31 - 1


def mat3_mul(A, B):
    C = np.zeros((3, 3), F)
    for r in range(3):
        for c in range(3):
            C[r, c] = (A[r, 0] * B[0, c] + A[r, 1] * B[1, c]) + A[r, 2] * B[2, c]
    return C


def mat3_vec(A, x):
    return np.array([(A[r, 0] * x[0] + A[r, 1] * x[1]) + A[r, 2] * x[2] for r in range(3)], F)


def sim3_transforms(kf1, kf2, s12, R12, t12):
    """:1233-1236 and the arguments of :1265 / :1274: ((sR21 R1w, sR21 t1w + t21), (sR12 R2w, sR12 t2w + t12))"""
    s12, R12, t12 = F(s12), np.asarray(R12, F).reshape(3, 3), np.asarray(t12, F)
    sR12 = (s12 * R12).astype(F)
    sR21 = (F(1.0 / float(s12)) * R12.T).astype(F)
    t21 = -mat3_vec(sR21, t12)
    return ((mat3_mul(sR21, kf1.Rcw), mat3_vec(sR21, kf1.tcw) + t21),
            (mat3_mul(sR12, kf2.Rcw), mat3_vec(sR12, kf2.tcw) + t12))


def keys_of(kf, mp_id):
    """MapPoint::GetIndexInKeyFrame: every key of the key frame that holds the map point, ascending"""
    return [int(i) for i in np.flatnonzero(kf.mp_id == mp_id)] if mp_id >= 0 else []


def already_matched(kf1, kf2, match12):
    """vbAlreadyMatched1 / 2 (:1246-1261) as bit masks over the camera index"""
    am1, am2 = np.zeros(len(kf1.keys), np.int64), np.zeros(len(kf2.keys), np.int64)
    for i in range(len(kf1.keys)):
        idx2 = int(match12[i])
        if idx2 < 0 or kf2.mp_id[idx2] < 0:  # vpMatches12[i] == NULL
            continue
        am1[i] |= 1 << int(kf1.cam_of_key[i])
        for k in keys_of(kf2, int(kf2.mp_id[idx2])):
            am2[k] |= 1 << int(kf2.cam_of_key[k])
    return am1, am2


def _round(x):
    """std::round of a float: half away from zero"""
    x = float(x)
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


def build_grid(kf, cam):
    """FrameBase::AssignFeaturesToGrid of one camera: {(cell x, cell y): [keys ascending]}"""
    b = kf.bounds[cam]
    winv, hinv = F(GRID_COLS) / (b[1] - b[0]), F(GRID_ROWS) / (b[3] - b[2])
    grid = {}
    for i in np.flatnonzero(kf.cam_of_key == cam):
        px, py = _round((kf.keys["x"][i] - b[0]) * winv), _round((kf.keys["y"][i] - b[2]) * hinv)
        if 0 <= px < GRID_COLS and 0 <= py < GRID_ROWS:
            grid.setdefault((px, py), []).append(int(i))
    return grid


def cam_project(cam, Pc):
    """camm::{Pinhole, Radtan, KB8}Camera::Project: double arithmetic on the float parameters, the result rounded to float"""
    x, y, z = (float(v) for v in Pc)
    fx, fy, cx, cy = (float(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    k = [float(v) for v in cam["dist"]]
    if cam["model"] == 1:
        nk = int(cam["num_k"])
        invz = 1 / z
        xn, yn = x * invz, y * invz
        x2, y2, xy = xn * xn, yn * yn, xn * yn
        r2 = x2 + y2
        fd, term = 1.0, 1.0
        for i in range(nk):
            term *= r2
            fd += k[i] * term
        p0, p1 = k[nk], k[nk + 1]
        xd = xn * fd + 2 * p0 * xy + p1 * (r2 + 2 * x2)
        yd = yn * fd + 2 * p1 * xy + p0 * (r2 + 2 * y2)
        return F(fx * xd + cx), F(fy * yd + cy)
    if cam["model"] == 2:
        r2 = x * x + y * y
        r = math.sqrt(r2)
        if r > float(F(1e-5)):
            th = math.atan2(r, z)
            t2 = th * th
            thd = k[3] * t2
            thd += k[2]
            thd *= t2
            thd += k[1]
            thd *= t2
            thd += k[0]
            thd *= t2
            thd += 1
            thd *= th
            return F(fx * (x * thd / r) + cx), F(fy * (y * thd / r) + cy)
    invz = 1.0 / z
    return F(fx * x * invz + cx), F(fy * y * invz + cy)


def project_stage(src, dst, Rcrw, tcrw, th, skip, check_viewing_angle=False):
    """the search of SearchByProjectionBase (:44-192) for the map points of src's keys in dst: best_idx (a key of dst, -1)
    and best_dist (INT_MAX) per (point, camera of dst).  skip[i]: bit c = pvbAlreadyMatched1[i][c]."""
    n, nc = len(src.keys), dst.n_cams
    best_idx, best_dist = np.full((n, nc), -1, np.int32), np.full((n, nc), INT_MAX, np.int32)
    R, t = np.asarray(Rcrw, F), np.asarray(tcrw, F)
    grids = [build_grid(dst, c) for c in range(nc)]
    th = F(th)
    for i in range(n):
        if src.mp_id[i] < 0:
            continue
        P = src.points[i]
        X = P["Xw"]
        Pcr = mat3_vec(R, X) + t
        for c in range(nc):
            if int(skip[i]) & (1 << c):
                continue
            Tc = dst.Tcr[c].reshape(3, 4)
            Pc = np.array([((Tc[r, 0] * Pcr[0] + Tc[r, 1] * Pcr[1]) + Tc[r, 2] * Pcr[2]) + Tc[r, 3] for r in range(3)], F)
            trc = dst.trc[c]
            twc = np.array([dst.Ow[r] + ((R[0, r] * trc[0] + R[1, r] * trc[1]) + R[2, r] * trc[2]) for r in range(3)], F)
            if Pc[2] <= 0:
                continue
            invz = F(1) / Pc[2]
            cam = dst.cams[c]
            if not dst.use_distort:
                p0, p1 = Pc[0] * invz, Pc[1] * invz
                u = (cam["fx"] * p0 + F(0) * p1) + cam["cx"] * F(1)
                v = (F(0) * p0 + cam["fy"] * p1) + cam["cy"] * F(1)
            else:
                u, v = cam_project(cam, Pc)
            b = dst.bounds[c]
            if not (b[0] <= u < b[1] and b[2] <= v < b[3]):
                continue
            PO = X - twc
            dist3D = np.sqrt((PO[0] * PO[0] + PO[1] * PO[1]) + PO[2] * PO[2])
            if dist3D < F(0.8) * P["min_distance"] or dist3D > F(1.2) * P["max_distance"]:
                continue
            if check_viewing_angle:
                nrm = P["normal"]
                if float((PO[0] * nrm[0] + PO[1] * nrm[1]) + PO[2] * nrm[2]) < 0.5 * float(dist3D):
                    continue
            ratio = P["max_distance"] / dist3D
            lvl = int(np.ceil(F(np.log(np.float64(ratio))) / dst.log_scale_factor))
            lvl = min(max(lvl, 0), dst.n_levels - 1)
            radius = th * dst.scale_factors[lvl]
            winv, hinv = F(GRID_COLS) / (b[1] - b[0]), F(GRID_ROWS) / (b[3] - b[2])
            x0 = max(0, int(np.floor((u - b[0] - radius) * winv)))
            x1 = min(GRID_COLS - 1, int(np.ceil((u - b[0] + radius) * winv)))
            y0 = max(0, int(np.floor((v - b[2] - radius) * hinv)))
            y1 = min(GRID_ROWS - 1, int(np.ceil((v - b[2] + radius) * hinv)))
            if x0 >= GRID_COLS or x1 < 0 or y0 >= GRID_ROWS or y1 < 0:
                continue
            bd, bi = INT_MAX, -1
            for ix in range(x0, x1 + 1):
                for iy in range(y0, y1 + 1):
                    for k in grids[c].get((ix, iy), ()):
                        kp = dst.keys[k]
                        if not (abs(kp["x"] - u) < radius and abs(kp["y"] - v) < radius):
                            continue
                        if kp["octave"] < lvl - 1 or kp["octave"] > lvl:
                            continue
                        d = int(np.unpackbits(P["desc"] ^ dst.desc[k]).sum())
                        if d < bd:
                            bd, bi = d, k
            best_idx[i, c], best_dist[i, c] = bi, bd
    return best_idx, best_dist


def only_one_match(src, dst, best_idx, best_dist, th_bestdist=TH_HIGH):
    """:204-225 with only1match and fuselater: vnMatch1[i] as the ascending list of dst's keys"""
    vn = [[] for _ in range(len(src.keys))]
    for i in range(len(src.keys)):
        if src.mp_id[i] < 0:
            continue
        bd, bi = INT_MAX, -1
        for c in range(dst.n_cams):
            if best_dist[i, c] < bd:
                if dst.mp_id[best_idx[i, c]] >= 0:
                    bd, bi = int(best_dist[i, c]), int(best_idx[i, c])
        if bd <= th_bestdist:
            vn[i] = keys_of(dst, int(dst.mp_id[bi]))
    return vn


def agreement(vn0, vn1, match12):
    """:1282-1298"""
    match12 = np.array(match12, np.int32)
    n_found = 0
    for i1, idx2s in enumerate(vn0):
        for idx2 in idx2s:
            if i1 in vn1[idx2]:
                match12[i1] = idx2
                n_found += 1
                break
    return match12, n_found


def search_by_sim3(kf1, kf2, s12, R12, t12, match12, th=7.5, detail=False):
    """int ORBmatcher::SearchBySim3: (match12 after the call, nFound)"""
    (R_a, t_a), (R_b, t_b) = sim3_transforms(kf1, kf2, s12, R12, t12)
    am1, am2 = already_matched(kf1, kf2, match12)
    fwd = project_stage(kf1, kf2, R_a, t_a, th, am1)
    bwd = project_stage(kf2, kf1, R_b, t_b, th, am2)
    vn0, vn1 = only_one_match(kf1, kf2, *fwd), only_one_match(kf2, kf1, *bwd)
    out, n_found = agreement(vn0, vn1, match12)
    if detail:
        return out, n_found, dict(fwd=fwd, bwd=bwd, vn=(vn0, vn1), am=(am1, am2), transforms=((R_a, t_a), (R_b, t_b)))
    return out, n_found


def search_by_sim3_brute(kf1, kf2, fwd, bwd, match12, th_bestdist=TH_HIGH):
    """The part after the two searches, written again from the reference's text with its own containers (sets of keys per
    point, a dictionary from map point to keys): the check on only_one_match / agreement."""
    def side(src, dst, best_idx, best_dist):
        holders = {}
        for k, m in enumerate(dst.mp_id):
            if m >= 0:
                holders.setdefault(int(m), set()).add(k)
        vn = []
        for i in range(len(src.keys)):
            s = set()
            if src.mp_id[i] >= 0:
                best_in_cams, idx_in_cams = INT_MAX, -1
                for cami in range(dst.n_cams):
                    bestDist, bestIdx = int(best_dist[i, cami]), int(best_idx[i, cami])
                    if bestIdx < 0:
                        continue  # no candidate passed: bestDist stays INT_MAX, never < bestDistInCams
                    if bestDist < best_in_cams:
                        if dst.mp_id[bestIdx] >= 0:
                            best_in_cams, idx_in_cams = bestDist, bestIdx
                if best_in_cams <= th_bestdist and dst.mp_id[idx_in_cams] >= 0:
                    s = set(holders[int(dst.mp_id[idx_in_cams])])
                    assert idx_in_cams in s  # CV_Assert(check)
            vn.append(s)
        return vn
    vn = [side(kf1, kf2, *fwd), side(kf2, kf1, *bwd)]
    out, n_found = np.array(match12, np.int32), 0
    for i1 in range(len(kf1.keys)):
        for idx2 in sorted(vn[0][i1]):
            if idx2 >= 0 and i1 in vn[1][idx2]:
                out[i1] = idx2
                n_found += 1
                break
    return out, n_found


# ---------------------------------------------------------------------------------------------------------------------
# the same search through the oracle's vo_fuse_search (per-camera key lists)
def oracle_project_stage(oracle, src, dst, Rcrw, tcrw, th, skip):
    from vieo_slam_amd.map_point import FUSE_FRAME_DTYPE
    FF = np.zeros(1, FUSE_FRAME_DTYPE)
    f = FF[0]["base"]
    f["Rcrw"], f["tcrw"], f["Ow"] = np.asarray(Rcrw, F).reshape(-1), tcrw, dst.Ow
    f["n_cams"], f["use_distort"], f["cams"] = dst.n_cams, dst.use_distort, dst.cams.ctypes.data
    f["Tcr"][:dst.n_cams], f["trc"][:dst.n_cams], f["bounds"][:dst.n_cams] = dst.Tcr, dst.trc, dst.bounds
    f["log_scale_factor"], f["n_levels"] = dst.log_scale_factor, dst.n_levels
    FF[0]["scale_factors"][:dst.n_levels] = dst.scale_factors
    FF[0]["inv_level_sigma2"][:dst.n_levels] = dst.inv_level_sigma2
    FF[0]["th_radius"] = th
    per_cam = [np.flatnonzero(dst.cam_of_key == c) for c in range(dst.n_cams)]
    pts = src.points.copy()
    pts["skip_mask"] = np.where(src.mp_id >= 0, np.asarray(skip, np.int64), -2 ** 31).astype(np.int32)
    bi, bd = oracle.fuse_search(FF, [dst.keys[k] for k in per_cam], [None] * dst.n_cams, [dst.desc[k] for k in per_cam], pts)
    bi = bi.copy()
    for c in range(dst.n_cams):
        hit = bi[:, c] >= 0
        bi[hit, c] = per_cam[c][bi[hit, c]]
    return bi, bd
