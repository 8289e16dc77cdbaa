"""Restatement of the matcher of the monocular initialisation, ORBmatcher::SearchForInitialization (reference
src/ORBmatcher.cc:628-723) with FrameBase::AssignFeaturesToGrid / GetFeaturesInArea (src/FrameBase.cpp:95-170), in numpy:
float32 operation by operation wherever the reference is float.  Two statements of the same function:

  search_for_initialization        the reference's loops as written: the grid as lists per cell, the window's cells column by
                                   column, the running bestDist / bestDist2, rotHist as lists
  search_for_initialization_brute  no grid and no running state: every key of the second frame tested against the window by
                                   its own cell, sorted by (cell, key); best and second best as order statistics of the
                                   candidates that are not skipped; the histogram as counts

tests/test_init_search_ref.py holds one against the other on tables that reach every branch, so that the restatement the GPU
tests compare with does not certify itself."""
import math

import numpy as np

f32 = np.float32
TH_LOW, HISTO_LENGTH = 50, 30
GRID_COLS, GRID_ROWS = 64, 48
INT_MAX = 2 ** 31 - 1

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(a, b):
    """DescriptorDistance of one 32-byte row against one or many"""
    return _POP[np.bitwise_xor(a, b)].sum(axis=-1)


def c_round(v):
    """round() of <cmath>: halves away from zero"""
    v = float(v)
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def grid_inv(bounds):
    b = np.asarray(bounds, f32)
    return f32(GRID_COLS) / (b[1] - b[0]), f32(GRID_ROWS) / (b[3] - b[2])


def pos_in_grid(x, y, bounds):
    """FrameBase::PosInGrid: the cell or None"""
    b = np.asarray(bounds, f32)
    winv, hinv = grid_inv(b)
    px, py = c_round((f32(x) - b[0]) * winv), c_round((f32(y) - b[2]) * hinv)
    if px < 0 or px >= GRID_COLS or py < 0 or py >= GRID_ROWS:
        return None
    return px, py


def assign_features_to_grid(keys, bounds):
    """vgrids_[0]: per cell (ix * ROWS + iy) the keys in push_back order"""
    cells = [[] for _ in range(GRID_COLS * GRID_ROWS)]
    for i in range(len(keys)):
        p = pos_in_grid(keys["x"][i], keys["y"][i], bounds)
        if p is not None:
            cells[p[0] * GRID_ROWS + p[1]].append(i)
    return cells


def cell_range(x, y, r, bounds):
    """the four cell bounds of GetFeaturesInArea, or None where it returns early"""
    b = np.asarray(bounds, f32)
    winv, hinv = grid_inv(b)
    x, y, r = f32(x), f32(y), f32(r)
    min_cx = max(0, int(math.floor(((x - b[0]) - r) * winv)))
    if min_cx >= GRID_COLS:
        return None
    max_cx = min(GRID_COLS - 1, int(math.ceil(((x - b[0]) + r) * winv)))
    if max_cx < 0:
        return None
    min_cy = max(0, int(math.floor(((y - b[2]) - r) * hinv)))
    if min_cy >= GRID_ROWS:
        return None
    max_cy = min(GRID_ROWS - 1, int(math.ceil(((y - b[2]) + r) * hinv)))
    if max_cy < 0:
        return None
    return min_cx, max_cx, min_cy, max_cy


def get_features_in_area(cells, keys, bounds, x, y, r, minlevel, maxlevel):
    """FrameBase::GetFeaturesInArea(0, x, y, r, minlevel, maxlevel) -> [(key, position in the walk over all keys of the cells)]"""
    rng = cell_range(x, y, r, bounds)
    out = []
    if rng is None:
        return out
    min_cx, max_cx, min_cy, max_cy = rng
    x, y, r = f32(x), f32(y), f32(r)
    checklevel = minlevel > 0 or maxlevel >= 0
    order = 0
    for ix in range(min_cx, max_cx + 1):
        for iy in range(min_cy, max_cy + 1):
            for j in cells[ix * GRID_ROWS + iy]:
                pos = order
                order += 1
                if checklevel:
                    if keys["octave"][j] < minlevel:
                        continue
                    if maxlevel >= 0 and keys["octave"][j] > maxlevel:
                        continue
                if abs(keys["x"][j] - x) < r and abs(keys["y"][j] - y) < r:
                    out.append((j, pos))
    return out


def rot_bin(a1, a2):
    rot = f32(a1) - f32(a2)
    if rot < 0.0:
        rot = rot + f32(360.0)
    b = c_round(rot * (f32(1.0) / f32(HISTO_LENGTH)))
    return 0 if b == HISTO_LENGTH else b


def compute_three_maxima(sizes):
    """ORBmatcher::ComputeThreeMaxima (:1608-1641) over the sizes of the bins -> (ind1, ind2, ind3)"""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if max2 < f32(0.1) * f32(max1):
        ind2 = ind3 = -1
    elif max3 < f32(0.1) * f32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def list_cut(nn_ratio):
    """the largest distance that can change an outcome of the walk: a larger one is no best (bestDist <= TH_LOW) and, as
    a second best, passes bestDist < (float)bestDist2 * mfNNratio for every bestDist <= TH_LOW"""
    cut = TH_LOW
    for d in range(TH_LOW + 1, 257):
        if not f32(d) * f32(nn_ratio) <= f32(TH_LOW):
            break
        cut = d
    return cut


def search_for_initialization(keys1, desc1, keys2, desc2, prev_matched, window_size, bounds, nn_ratio=0.9, check_orientation=True):
    """-> dict(matches12, nmatches, prev_matched (a copy, updated), lists (per key of F1 the [(key, dist, order)] with
    dist <= list_cut, what the device hands to the host), stats (how often each branch was taken))"""
    n1, n2 = len(keys1), len(keys2)
    nn = f32(nn_ratio)
    cut = list_cut(nn_ratio)
    prev = np.array(prev_matched, f32).reshape(n1, 2)
    cells = assign_features_to_grid(keys2, bounds)
    matches12 = np.full(n1, -1, np.int32)
    matched_distance = [INT_MAX] * n2
    matches21 = [-1] * n2
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    stats = dict(steal=0, skip_equal=0, skip_less=0, empty=0, octave=0, erased=0, ratio_fail=0, over_low=0, second_over_low=0)
    lists = [[] for _ in range(n1)]
    for i1 in range(n1):
        level1 = int(keys1["octave"][i1])
        if level1 > 0:
            stats["octave"] += 1
            continue
        ind2 = get_features_in_area(cells, keys2, bounds, prev[i1, 0], prev[i1, 1], window_size, level1, level1)
        if not ind2:
            stats["empty"] += 1
            continue
        best, best2, best_idx = INT_MAX, INT_MAX, -1
        for i2, pos in ind2:
            dist = int(hamming(desc1[i1], desc2[i2]))
            if dist <= cut:
                lists[i1].append((i2, dist, pos))
            if matched_distance[i2] <= dist:
                stats["skip_equal" if matched_distance[i2] == dist else "skip_less"] += 1
                continue
            if dist < best:
                best2, best, best_idx = best, dist, i2
            elif dist < best2:
                best2 = dist
        if best <= TH_LOW:
            if f32(best) < f32(best2) * nn:
                if matches21[best_idx] >= 0:
                    matches12[matches21[best_idx]] = -1
                    nmatches -= 1
                    stats["steal"] += 1
                matches12[i1] = best_idx
                matches21[best_idx] = i1
                matched_distance[best_idx] = best
                nmatches += 1
                if best2 != INT_MAX and best2 > TH_LOW:
                    stats["second_over_low"] += 1
                if check_orientation:
                    rot_hist[rot_bin(keys1["angle"][i1], keys2["angle"][best_idx])].append(i1)
            else:
                stats["ratio_fail"] += 1
        elif best != INT_MAX:
            stats["over_low"] += 1
    if check_orientation:
        keep = compute_three_maxima([len(h) for h in rot_hist])
        for i in range(HISTO_LENGTH):
            if i in keep:
                continue
            for idx1 in rot_hist[i]:
                if matches12[idx1] >= 0:
                    matches12[idx1] = -1
                    nmatches -= 1
                    stats["erased"] += 1
    for i1 in range(n1):
        if matches12[i1] >= 0:
            prev[i1, 0], prev[i1, 1] = keys2["x"][matches12[i1]], keys2["y"][matches12[i1]]
    return dict(matches12=matches12, nmatches=nmatches, prev_matched=prev, lists=lists, stats=stats)


def search_for_initialization_brute(keys1, desc1, keys2, desc2, prev_matched, window_size, bounds, nn_ratio=0.9,
                                    check_orientation=True):
    """the second statement -> (matches12, nmatches, prev_matched)"""
    n1, n2 = len(keys1), len(keys2)
    prev = np.array(prev_matched, f32).reshape(n1, 2)
    b = np.asarray(bounds, f32)
    winv, hinv = grid_inv(b)
    # the cell of every key of F2 (halves away from zero, in double on the exact float32 value), -1 outside the grid
    vx, vy = ((keys2["x"].astype(f32) - b[0]) * winv).astype(np.float64), ((keys2["y"].astype(f32) - b[2]) * hinv).astype(np.float64)
    cx = (np.sign(vx) * np.floor(np.abs(vx) + 0.5)).astype(np.int64)
    cy = (np.sign(vy) * np.floor(np.abs(vy) + 0.5)).astype(np.int64)
    in_grid = (cx >= 0) & (cx < GRID_COLS) & (cy >= 0) & (cy < GRID_ROWS)
    walk = np.lexsort((np.arange(n2), cy, cx))  # cell column, cell row, key
    r = f32(window_size)
    holder = {}  # key of F2 -> (key of F1 that holds it, its distance)
    pushes = []  # (key of F1, bin) of every accepted match, in order
    for i1 in range(n1):
        if keys1["octave"][i1] > 0:
            continue
        rng = cell_range(prev[i1, 0], prev[i1, 1], r, b)
        if rng is None:
            continue
        ok = in_grid & (cx >= rng[0]) & (cx <= rng[1]) & (cy >= rng[2]) & (cy <= rng[3]) & (keys2["octave"] == 0)
        ok &= (np.abs(keys2["x"].astype(f32) - prev[i1, 0]) < r) & (np.abs(keys2["y"].astype(f32) - prev[i1, 1]) < r)
        cand = [j for j in walk if ok[j]]
        if not cand:
            continue
        d = hamming(desc1[i1][None, :], desc2[cand]) if cand else np.zeros(0, np.int32)
        live = [(int(dd), k) for k, (j, dd) in enumerate(zip(cand, d)) if not (j in holder and holder[j][1] <= dd)]
        if not live:
            continue
        live.sort()  # by distance, then by position in the walk
        best, best_idx = live[0][0], cand[live[0][1]]
        second = live[1][0] if len(live) > 1 else INT_MAX
        if best <= TH_LOW and f32(best) < f32(second) * f32(nn_ratio):
            holder[best_idx] = (i1, best)
            pushes.append((i1, rot_bin(keys1["angle"][i1], keys2["angle"][best_idx])))
    matches12 = np.full(n1, -1, np.int32)
    for j, (i1, _) in holder.items():
        matches12[i1] = j
    if check_orientation:
        counts = np.bincount([bn for _, bn in pushes], minlength=HISTO_LENGTH)
        # the three fullest bins, the earlier bin first among equals (the reference's comparisons are strict); the second
        # and third only with at least a tenth of the first, the third only if the second stays
        top = [i for i in sorted(range(HISTO_LENGTH), key=lambda i: (-counts[i], i)) if counts[i] > 0][:3]
        keep = top[:1]
        if len(top) > 1 and not counts[top[1]] < f32(0.1) * f32(counts[top[0]]):
            keep = top[:2]
            if len(top) > 2 and not counts[top[2]] < f32(0.1) * f32(counts[top[0]]):
                keep = top[:3]
        for i1, bn in pushes:
            if bn not in keep:
                matches12[i1] = -1
    for i1 in np.nonzero(matches12 >= 0)[0]:
        prev[i1] = keys2["x"][matches12[i1]], keys2["y"][matches12[i1]]
    return matches12, int((matches12 >= 0).sum()), prev
