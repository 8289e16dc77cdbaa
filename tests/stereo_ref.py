"""Frame::ComputeStereoMatches (reference src/Frame.cc:451-611) restated in numpy / plain Python from the reference
text, with a census: one record per left key that says how far the key got and through which values.  Test
infrastructure only.  The float roundings are the reference's: float products and sums (np.float32 scalars), C round()
(half away from zero), the (int) casts of rowRange / colRange, cv::norm(NORM_L1) of small integers (exact), the double
`uL - 0.01`.

    uright, depth, census = compute_stereo_matches(planes_l, planes_r, kl, dl, kr, dr, scale, inv_scale, baseline, bf)

planes_*: the pyramid planes of the two extractors (OracleExtractor.plane(l, 0)), scale / inv_scale float32 per level.
census[i] is a dict:
    row          (int) y of the left key                 n_cand    right keys in vRowIndices[row]
    n_gated      candidates inside the octave gate and [minU, maxU]
    best_dist    best descriptor distance (TH_HIGH if no candidate beat it), best_idx its right key (-1: none)
    tied         right keys at best_dist among the gated candidates (len > 1: a tie, the lowest index wins)
    gate         where the key ended, one of GATES
    sads         the 11 SADs (None before the refinement), best_inc, delta_r, zero_branch (disparity <= 0 taken)
    sad          the best SAD (accepted and median-rejected keys)
and the frame's median / threshold sit in census.median, census.th_dist (None without an accepted match).
"""
import numpy as np

TH_HIGH, TH_LOW = 100, 50
GATES = ("no_candidate", "maxU<0", "bestDist>=75", "endu>=cols", "bestincR=-L", "bestincR=+L", "deltaR", "disparity",
         "median", "accepted")
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
f32 = np.float32


class Census(list):
    median = None
    th_dist = None
    n_accepted = 0  # before the median rejection

    def count(self, gate):
        return sum(1 for r in self if r["gate"] == gate)

    def gates(self):
        return {g: self.count(g) for g in GATES}


def c_round(x):
    """C round() of a float: half away from zero (the float -> double conversion is exact)."""
    x = float(x)
    return f32(np.floor(x + 0.5) if x >= 0 else -np.floor(-x + 0.5))


def hamming(a, b):
    return int(_POP[np.bitwise_xor(a, b)].sum())


def row_indices(kr, scale, n_rows):
    """vRowIndices (Frame.cc:461-480): per image row the right keys whose band covers it, in key order."""
    rows = [[] for _ in range(n_rows)]
    for ir in range(len(kr)):
        y = f32(kr["y"][ir])
        r = f32(2.0) * f32(scale[int(kr["octave"][ir])])
        maxr, minr = int(np.ceil(f32(y + r))), int(np.floor(f32(y - r)))
        for yi in range(max(minr, 0), min(maxr, n_rows - 1) + 1):
            rows[yi].append(ir)
    return rows


def compute_stereo_matches(planes_l, planes_r, kl, dl, kr, dr, scale, inv_scale, baseline, bf):
    n = len(kl)
    uright, depth = np.full(n, -1, np.float32), np.full(n, -1, np.float32)
    census = Census()
    th_orb = (TH_HIGH + TH_LOW) // 2
    n_rows = planes_l[0].shape[0]
    rows = row_indices(kr, scale, n_rows)
    dl = np.asarray(dl, np.uint8).reshape(-1, 32)
    dr = np.asarray(dr, np.uint8).reshape(-1, 32)
    kr_x = np.asarray(kr["x"], np.float32)
    kr_oct = np.asarray(kr["octave"], np.int64)
    baseline, bf = f32(baseline), f32(bf)
    min_d, max_d = f32(0), f32(bf / baseline)
    dist_idx = []
    w, L = 5, 5
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for il in range(n):
            level = int(kl["octave"][il])
            vl, ul = f32(kl["y"][il]), f32(kl["x"][il])
            rec = dict(row=int(vl), n_cand=0, n_gated=0, best_dist=TH_HIGH, best_idx=-1, tied=[], gate=None, sads=None,
                       best_inc=None, delta_r=None, zero_branch=False, sad=None)
            census.append(rec)
            cand = rows[int(vl)]
            rec["n_cand"] = len(cand)
            if not cand:
                rec["gate"] = "no_candidate"
                continue
            min_u, max_u = f32(ul - max_d), f32(ul - min_d)
            if max_u < 0:
                rec["gate"] = "maxU<0"
                continue
            c = np.asarray(cand, np.int64)
            ok = (kr_oct[c] >= level - 1) & (kr_oct[c] <= level + 1) & (kr_x[c] >= min_u) & (kr_x[c] <= max_u)
            c = c[ok]
            rec["n_gated"] = len(c)
            best_dist, best_idx = TH_HIGH, 0
            if len(c):
                d = _POP[np.bitwise_xor(dr[c], dl[il][None, :])].sum(axis=1)
                k = int(np.argmin(d))  # (the first of equal distances: candidates are in key order)
                if d[k] < best_dist:
                    best_dist, best_idx = int(d[k]), int(c[k])
                    rec["best_dist"], rec["best_idx"] = best_dist, best_idx
                    rec["tied"] = [int(j) for j in c[d == d[k]]]
            if not best_dist < th_orb:
                rec["gate"] = "bestDist>=75"
                continue
            ur0 = f32(kr_x[best_idx])
            sf = f32(inv_scale[level])
            su_l, sv_l, su_r0 = c_round(f32(ul * sf)), c_round(f32(vl * sf)), c_round(f32(ur0 * sf))
            pl, pr = planes_l[level], planes_r[level]
            r0, c0 = int(f32(sv_l - w)), int(f32(su_l - w))
            assert r0 >= 0 and c0 >= 0 and r0 + 11 <= pl.shape[0] and c0 + 11 <= pl.shape[1], "left patch outside its level"
            il_patch = pl[r0:r0 + 11, c0:c0 + 11].astype(np.int64) - int(pl[r0 + w, c0 + w])
            iniu, endu = f32(su_r0 + L - w), f32(su_r0 + L + w + 1)
            if iniu < 0 or endu >= pr.shape[1]:
                rec["gate"] = "endu>=cols"
                continue
            best_s, best_inc, sads = None, 0, []
            for inc in range(-L, L + 1):
                cc = int(f32(f32(su_r0 + inc) - w))
                assert cc >= 0, "right strip starts left of the plane (out of domain)"
                ir_patch = pr[r0:r0 + 11, cc:cc + 11].astype(np.int64) - int(pr[r0 + w, cc + w])
                s = int(np.abs(il_patch - ir_patch).sum())
                if best_s is None or s < best_s:
                    best_s, best_inc = s, inc
                sads.append(s)
            rec["sads"], rec["best_inc"] = sads, best_inc
            if best_inc == -L or best_inc == L:
                rec["gate"] = "bestincR=-L" if best_inc == -L else "bestincR=+L"
                continue
            d1, d2, d3 = f32(sads[L + best_inc - 1]), f32(sads[L + best_inc]), f32(sads[L + best_inc + 1])
            delta = f32(f32(d1 - d3) / f32(f32(2.0) * f32(f32(d1 + d3) - f32(f32(2.0) * d2))))
            rec["delta_r"] = delta
            if delta < -1 or delta > 1:
                rec["gate"] = "deltaR"
                continue
            best_ur = f32(f32(scale[level]) * f32(f32(su_r0 + f32(best_inc)) + delta))
            disparity = f32(ul - best_ur)
            if disparity >= min_d and disparity < max_d:
                if disparity <= 0:
                    rec["zero_branch"] = True
                    disparity = f32(0.01)
                    best_ur = f32(float(ul) - 0.01)
                depth[il] = f32(bf / disparity)
                uright[il] = best_ur
                rec["gate"], rec["sad"] = "accepted", best_s
                dist_idx.append((best_s, il))
            else:
                rec["gate"] = "disparity"  # (a NaN deltaR ends here too: every comparison with it is false)
    census.n_accepted = len(dist_idx)
    if not dist_idx:
        return uright, depth, census
    dist_idx.sort()
    median = f32(dist_idx[len(dist_idx) // 2][0])
    th = f32(f32(f32(1.5) * f32(1.4)) * median)
    census.median, census.th_dist = float(median), float(th)
    for s, il in reversed(dist_idx):
        if f32(s) < th:
            break
        uright[il] = depth[il] = -1
        census[il]["gate"] = "median"
    return uright, depth, census
