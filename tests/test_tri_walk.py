"""The host half of SearchForTriangulation and of the triangulation that follows it (vieo_slam_amd/csrc/tri_walk.h):
the entries' checks, the query plan, the order-dependent walk, the row gather and the result scatter.  CPU only: the
header is compiled with g++ (tests/emul/tri_walk_emul.cc).  The candidate table k_tri_gates writes on the device is
built here by asking the oracle's vo_tri_gates for every (query, node key of pKF2) the kernel would visit; the device
fills it in test_tri_search.py and test_new_points.py.

What the walk has to decide is established apart from the code under test: `walk_ref` below restates the walk over the
same table with dictionaries where the header keeps vectors, is itself held against the oracle's rows in every case,
and counts the situations it meets."""
import collections
import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from tests import new_points_ref, reloc_ref
from vieo_slam_amd import tri_search
from vieo_slam_amd.tri_search import NEWPT_SKIPPED, TriKeyFrame, TriStereo

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
VIEO_OK, VIEO_E_INVALID, VIEO_E_CAPACITY = 0, -1, -4
TH_LOW, HISTO_LENGTH = reloc_ref.TH_LOW, reloc_ref.HISTO_LENGTH
BF = 47.9
f32 = np.float32
V, I = ctypes.c_void_p, ctypes.c_int


@functools.lru_cache(maxsize=None)
def lib():
    out = os.path.join(HERE, "emul", "libtri_walk_emul.so")
    csrc = os.path.join(ROOT, "vieo_slam_amd", "csrc")
    deps = [os.path.join(HERE, "emul", "tri_walk_emul.cc")] + [os.path.join(csrc, h) for h in (
        "tri_walk.h", "bow_walk.h", "match_groups.h", "orb_match.h")] + [os.path.join(ROOT, "include", "vieo_hot.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-o", out, deps[0]])
    L = ctypes.CDLL(out)
    L.tw_error.restype = ctypes.c_char_p
    L.tw_plan.argtypes = [V] * 4 + [I] * 3 + [V] * 8 + [I] + [V] * 3
    L.tw_walk.argtypes = [V, V, I, I, I, I] + [V] * 5
    L.tw_gather.argtypes = [V] * 4 + [I] * 3 + [V] * 9
    L.tw_scatter.argtypes = [I, I] + [V] * 7
    L.tw_scatter.restype = None
    L.tw_fill_compare.argtypes = [I, I, V, I, V]
    return L


def p(a):
    return a.ctypes.data_as(V) if a is not None and a.size else None


def recs(items):
    return np.concatenate([k.rec for k in items])


def stride_of(kf1, kf2s):
    return kf1.n_cams + max(k.n_cams for k in kf2s)


Plan = collections.namedtuple("Plan", "rc queries q_begin offs n_cand")


def plan(kf1, kf2s, only_stereo=False, stereo=None, stride=None):
    """the checks and the plan of vieo_search_for_triangulation, or with stereo = (st1, st2s) of vieo_create_new_map_points"""
    n = len(kf2s)
    cap_q = len(kf1.node_feat) * n + 1  # a feature of pKF1 is a query once per neighbour at the most
    q, qb, offs, nc = np.zeros((cap_q, 5), np.int32), np.zeros(n + 1, np.int32), np.zeros((4, n + 2), np.int32), np.zeros(1, np.int64)
    dummy = np.zeros(16, np.float64)
    st = [None, None] if stereo is None else [p(stereo[0].rec), p(recs(stereo[1]))]
    rc = lib().tw_plan(p(kf1.rec), st[0], p(recs(kf2s)), st[1], n, int(only_stereo), stride or stride_of(kf1, kf2s),
                       *[p(dummy)] * 7, p(q), cap_q, p(qb), p(offs), p(nc))
    return Plan(rc, q[:max(rc, 0)], qb, offs, int(nc[0]))


def expected_queries(kf1, kf2s, only_stereo, skipped=()):
    """(idx1, pair, first2, count2) in the reference's order, from the shared nodes as Python sees them"""
    out = []
    for pr, kf2 in enumerate(kf2s):
        if pr in skipped:
            continue
        at2 = {int(nd): k for k, nd in enumerate(kf2.node_id)}
        for k1, nd in enumerate(kf1.node_id):
            k2 = at2.get(int(nd))
            if k2 is None or kf2.node_first[k2 + 1] == kf2.node_first[k2]:
                continue
            for idx1 in kf1.node_feat[kf1.node_first[k1]:kf1.node_first[k1 + 1]]:
                if not kf1.has_mp[idx1] and not (only_stereo and not kf1.uright[idx1] >= 0):
                    out.append((int(idx1), pr, int(kf2.node_first[k2]), int(kf2.node_first[k2 + 1] - kf2.node_first[k2])))
    return out


def gates_table(oracle, kf1, kf2s, P, only_stereo):
    """what k_tri_gates writes: per query the (idx2, dist) of the node's keys of pKF2 that hold no map point, are stereo
    under only_stereo and pass vo_tri_gates, in the node's order"""
    oracle.tri_gates(kf1, kf2s[0], 0, 0)  # (binds the function)
    gates = oracle.L.vo_tri_gates
    cand, cand_n = np.full((P.n_cand + 1, 2), -9, np.int32), np.zeros(len(P.queries), np.int32)
    for q, (idx1, pr, first2, count2, out_off) in enumerate(P.queries.tolist()):
        kf2, n = kf2s[pr], 0
        for idx2 in kf2.node_feat[first2:first2 + count2].tolist():
            if kf2.has_mp[idx2] or (only_stereo and not kf2.uright[idx2] >= 0):
                continue
            d = gates(kf1.rec.ctypes.data, kf2.rec.ctypes.data, idx1, idx2, None)
            if d >= 0:
                cand[out_off + n] = idx2, d
                n += 1
        cand_n[q] = n
    return cand, cand_n


def walk(kf1, kf2s, cand, cand_n, check=True, cap=None, stride=None):
    """tw_walk over the plan the last plan() left; raw buffers, unwritten rows stay 7, one guard block behind the last"""
    n = len(kf2s)
    cap = int(cap if cap is not None else max(2 * len(kf1.keys), 1))
    stride = stride or stride_of(kf1, kf2s)
    pairs = np.full((n + 1, cap, stride), 7, np.int32)
    n_pairs, n_matches = np.full(n, -5, np.int32), np.full(n, -5, np.int32)
    rc = lib().tw_walk(p(kf1.rec), p(recs(kf2s)), n, int(check), cap, stride, p(cand), p(cand_n), p(pairs), p(n_pairs), p(n_matches))
    return rc, pairs, n_pairs, n_matches


# ---------------------------------------------------------------------------------------------------------------------
# the walk restated (ORBmatcher.cc:962-1146 and camera_base.h:408-574 as oracle/tri_search.cc has them)
def _rot_bin(a1, a2):
    rot = f32(a1) - f32(a2)
    if rot < 0.0:
        rot = f32(rot + f32(360.0))
    b = int(math.floor(float(f32(rot * (f32(1.0) / f32(HISTO_LENGTH)))) + 0.5))
    return 0 if b == HISTO_LENGTH else b


def _fill(idx, last, where, good, nc, ci, i, cj, j, dist, ev):
    ki, kj = (ci, i), (cj, j)
    gi, gj = where.get(ki), where.get(kj)
    if gi is None and gj is not None:
        gi = gj
    cam, key, check, contradict = (ci, cj), (i, j), [0, 0], 0
    if gi is None:
        g = len(good)
        idx.append([-1] * nc), last.append([math.inf] * nc), good.append(True)
        idx[g][ci], idx[g][cj], last[g][ci], last[g][cj] = i, j, dist, dist
        where[ki] = where[kj] = g
        return True
    g = gi
    if gj is not None and gj != g:
        contradict = 2
        mine, other = [last[g][t] for t in range(nc) if idx[g][t] != -1], [last[gj][t] for t in range(nc) if idx[gj][t] != -1]
        if sum(other) * len(mine) < sum(mine) * len(other):  # the smaller mean distance keeps its group
            g, contradict = gj, 1
    for t in (0, 1):
        if idx[g][cam[t]] == -1 or (key[t] != idx[g][cam[t]] and last[g][cam[t]] > dist):
            check[t] = 2
    if not any(check):
        return False
    if contradict:
        ev["contradiction, the other group wins" if contradict == 1 else "contradiction, the first group wins"] += 1
        gc = gi if contradict == 1 else gj
        for t in (0, 1):
            if key[t] == idx[gc][cam[t]]:
                where.pop((cam[t], key[t]), None)
                last[gc][cam[t]], idx[gc][cam[t]] = math.inf, -1
    for t in (0, 1):
        if check[t] == 2:
            if key[t] != idx[g][cam[t]]:
                if idx[g][cam[t]] != -1:
                    ev["displaced"] += 1
                    where.pop((cam[t], idx[g][cam[t]]), None)
                where.setdefault((cam[t], key[t]), g)
                idx[g][cam[t]] = key[t]
            last[g][cam[t]] = dist
        elif last[g][cam[t]] > dist:
            last[g][cam[t]] = dist
    return True


def walk_ref(kf1, kf2, queries, cand, cand_n, check):
    """(rows, nmatches, events) of one neighbour; queries: this neighbour's rows of the plan, cand_n: their counts"""
    rig = hasattr(kf1, "key_cam")
    nc1, nc = kf1.n_cams, kf1.n_cams + kf2.n_cams
    cam = (lambda k, i: int(k.key_cam[i])) if rig else (lambda k, i: 0)
    idx, last, where, good, ev = [], [], {}, [], collections.Counter()
    hist, nm = [[] for _ in range(HISTO_LENGTH)], 0
    for (idx1, _, _, _, out_off), n in zip(queries.tolist(), cand_n.tolist()):
        c1, free = cam(kf1, idx1), collections.defaultdict(list)
        for idx2, d in cand[out_off:out_off + n].tolist():
            g = where.get((nc1 + cam(kf2, idx2), idx2))
            if g is not None and idx[g][c1] != -1:
                ev["taken"] += 1
            else:
                free[cam(kf2, idx2)].append((idx2, d))
        for img in sorted(free):
            best = min(d for _, d in free[img])
            at_best = [i2 for i2, d in free[img] if d == best]
            ev["tie"] += len(at_best) > 1
            ev["second image"] += img != sorted(free)[0]
            if _fill(idx, last, where, good, nc, c1, idx1, nc1 + img, at_best[-1], best, ev):
                nm += 1
            if check:
                hist[_rot_bin(kf1.keys["angle"][idx1], kf2.keys["angle"][at_best[-1]])].append(idx1)
    if check:
        keep = reloc_ref.three_maxima([len(h) for h in hist])
        for b in range(HISTO_LENGTH):
            for idx1 in hist[b] if b not in keep else []:
                g = where.get((cam(kf1, idx1), idx1))
                if g is not None:
                    good[g], nm = False, nm - 1
                    ev["rotation"] += 1
    rows = []
    for g in range(len(good)):
        if sum(v != -1 for v in idx[g]) < 2:
            ev["one member"] += good[g]
        elif good[g]:
            rows.append(idx[g])
    return np.array(rows, np.int32).reshape(-1, nc), nm, ev


# ---------------------------------------------------------------------------------------------------------------------
SCENES = {
    "default": (20, {}, False, True),
    "only_stereo": (21, {}, True, True),
    "no_orientation": (22, {}, False, False),
    "lookalikes": (23, dict(n_nodes=60, dup_frac=0.5, flip_bits=4), False, True),
    "radtan": (24, dict(rig="radtan", n_points=500), False, True),
    "kb8": (25, dict(rig="kb8", n_neighbours=4, n_points=500), False, True),
}
_events = collections.Counter()


def run_case(oracle, kf1, kf2s, only_stereo, check, events=None):
    """plan, table, walk; the header against the oracle and the restatement; returns the plan and the table"""
    P = plan(kf1, kf2s, only_stereo)
    want_q = expected_queries(kf1, kf2s, only_stereo)
    assert P.rc == len(want_q) == len(P.queries)
    assert [tuple(r) for r in P.queries[:, :4].tolist()] == want_q
    assert P.queries[:, 4].tolist() == np.concatenate([[0], np.cumsum(P.queries[:, 3])[:-1]]).tolist()[:len(want_q)]
    assert P.n_cand == P.queries[:, 3].sum()
    assert P.q_begin.tolist() == [int((P.queries[:, 1] < pr).sum()) for pr in range(len(kf2s) + 1)]
    cand, cand_n = gates_table(oracle, kf1, kf2s, P, only_stereo)
    rc, pairs, n_pairs, n_matches = walk(kf1, kf2s, cand, cand_n, check)
    assert rc == VIEO_OK, lib().tw_error()
    ref = oracle.search_for_triangulation(kf1, kf2s, only_stereo, check)
    for pr, (kf2, (rows, nm)) in enumerate(zip(kf2s, ref)):
        nc = kf1.n_cams + kf2.n_cams
        assert n_pairs[pr] == len(rows) and n_matches[pr] == nm, pr
        assert np.array_equal(pairs[pr, :len(rows), :nc], rows), pr
        assert (pairs[pr, :len(rows), nc:] == -1).all() and (pairs[pr, len(rows):] == 7).all()
        r_rows, r_nm, ev = walk_ref(kf1, kf2, P.queries[P.q_begin[pr]:P.q_begin[pr + 1]], cand, cand_n[P.q_begin[pr]:P.q_begin[pr + 1]], check)
        assert np.array_equal(r_rows, rows) and r_nm == nm, pr  # the restatement, before its counts are believed
        if events is not None:
            events.update({k: v for k, v in ev.items() if v})
    return P, cand, cand_n


@pytest.mark.parametrize("name", list(SCENES))
def test_plan_and_walk_against_the_oracle(oracle, name):
    seed, kw, only_stereo, check = SCENES[name]
    kf1, kf2s, _ = tri_search.make_tri_scene(seed, **dict(dict(n_points=900, n_neighbours=3), **kw))
    assert 2 <= len(kf2s) <= 4
    ev = collections.Counter()
    P, _, cand_n = run_case(oracle, kf1, kf2s, only_stereo, check, ev)
    assert len(P.queries) > 100 and cand_n.sum() > 50
    # the offsets: pKF1 first, then the neighbours; node_feat lists of the neighbours only
    frames = [kf1] + kf2s
    assert P.offs[0].tolist() == np.concatenate([[0], np.cumsum([len(k.keys) for k in frames])]).tolist()
    assert P.offs[1].tolist() == np.concatenate([[0, 0], np.cumsum([len(k.node_feat) for k in kf2s])]).tolist()
    assert P.offs[2].tolist() == np.concatenate([[0], np.cumsum([len(k.scale) for k in frames])]).tolist()
    assert not P.offs[3].any()
    _events.update({(name, k): v for k, v in ev.items()})
    print(name, dict(ev))


def rebuilt(kf, keys=None, desc=None, uright=None, has_mp=None, feat_vec=None):
    """a copy of an undistorted key frame with some arrays replaced"""
    T = np.eye(4)
    T[:3] = kf.rec[0]["Tcw"].reshape(3, 4)
    fv = [(int(n), kf.node_feat[kf.node_first[k]:kf.node_first[k + 1]].tolist()) for k, n in enumerate(kf.node_id)]
    pick = lambda a, b: b if a is None else a
    return TriKeyFrame(T, tuple(kf.rec[0][k] for k in ("fx", "fy", "cx", "cy")), pick(keys, kf.keys), pick(desc, kf.desc),
                       pick(uright, kf.uright), pick(has_mp, kf.has_mp), pick(feat_vec, fv), kf.scale, kf.sigma2)


def test_planted_tie_goes_to_the_later_key(oracle):
    """a second key of pKF2 with the place and descriptor of a matched one, behind it in its node: same gates, same
    distance, and the reference's `dist > bestDist: continue` lets the later one replace the earlier"""
    kf1, kf2s, _ = tri_search.make_tri_scene(26, n_points=300, n_neighbours=2, n_nodes=100)
    rows = oracle.search_for_triangulation(kf1, kf2s)[1][0]
    kf2 = kf2s[1]
    i1, i2 = (int(v) for v in rows[len(rows) // 2])
    n = len(kf2.keys)
    fv = [(int(nd), kf2.node_feat[kf2.node_first[k]:kf2.node_first[k + 1]].tolist()) for k, nd in enumerate(kf2.node_id)]
    fv = [(nd, f + [n] if i2 in f else f) for nd, f in fv]
    twin = rebuilt(kf2, np.append(kf2.keys, kf2.keys[i2:i2 + 1]), np.append(kf2.desc, kf2.desc[i2:i2 + 1], 0),
                   np.append(kf2.uright, kf2.uright[i2]), np.append(kf2.has_mp, 0), fv)
    ev = collections.Counter()
    run_case(oracle, kf1, [kf2s[0], twin], False, True, ev)
    assert [i1, n] in oracle.search_for_triangulation(kf1, [kf2s[0], twin])[1][0].tolist() and ev["tie"] >= 1
    _events.update({("planted tie", k): v for k, v in ev.items()})


def test_planted_displacement_on_a_rig(oracle):
    """A scene point that two cameras of pKF1 (keys k3, then k1 in their node) and two images a < b of pKF2 (keys ka, kb)
    see is one row {k3, k1, ka, kb}.  Planted: kb 5 bits from k3's descriptor, and another key of image b in kb's node
    made a twin of kb with k1's own descriptor.  k3 takes ka and kb (5 < its distance to the twin); k1 joins the group
    through ka, and for image b brings the twin at distance 0 < 5: kb is displaced from the group."""
    kf1, kf2s, _ = tri_search.make_tri_scene(31, rig="kb8", n_points=500, n_neighbours=2, n_nodes=40)
    kf2, nc1 = kf2s[0], kf1.n_cams
    rows = oracle.search_for_triangulation(kf1, [kf2])[0][0]
    in_rows = set(rows[:, nc1:].reshape(-1).tolist())
    place1 = {int(i): n for n, i in enumerate(kf1.node_feat)}
    node2 = np.repeat(np.arange(len(kf2.node_id)), np.diff(kf2.node_first))[np.argsort(kf2.node_feat, kind="stable")]
    planted = None
    for row in rows.tolist():
        k1s, k2s = sorted((i for i in row[:nc1] if i >= 0), key=place1.get), [i for i in row[nc1:] if i >= 0]
        if len(k1s) < 2 or len(k2s) < 2:
            continue
        (k3, k1), (ka, kb) = k1s[:2], k2s[:2]
        b = int(kf2.key_cam[kb])
        node = kf2.node_feat[kf2.node_first[node2[kb]]:kf2.node_first[node2[kb] + 1]].tolist()
        victims = [v for v in node if kf2.key_cam[v] == b and v not in in_rows and not kf2.has_mp[v]]
        if victims and int(np.unpackbits(kf1.desc[k3] ^ kf1.desc[k1]).sum()) > 5:
            planted = k3, k1, ka, kb, victims[0]
            break
    assert planted is not None
    k3, k1, ka, kb, twin = planted
    kf2.desc[kb] = kf1.desc[k3]
    kf2.desc[kb, 0] ^= 0x1F
    kf2.keys[twin], kf2.uright[twin], kf2.desc[twin] = kf2.keys[kb], kf2.uright[kb], kf1.desc[k1]
    ev = collections.Counter()
    run_case(oracle, kf1, [kf2, kf2s[1]], False, True, ev)
    got = oracle.search_for_triangulation(kf1, [kf2])[0][0]
    assert ev["displaced"] >= 1 and kb not in got[:, nc1:]
    assert {k3, k1} <= set(got[got[:, nc1 + b] == twin][0, :nc1].tolist())  # the twin sits with both keys of pKF1
    _events.update({("planted displacement", k): v for k, v in ev.items()})


@pytest.mark.parametrize("nc, n_keys", [(2, 6), (3, 5), (5, 4), (8, 4), (8, 40)])
def test_fe_fill_against_its_earlier_text(nc, n_keys):
    """fe_fill is order-dependent bookkeeping whose two per-side blocks were folded into loops.  Random sequences of
    pairs -- few keys, so that groups collide -- go through it and through the earlier text, which the emulation keeps word
    for word; the return value and every table must agree after every pair.  What the sequences met is counted from the
    earlier text's tables alone."""
    rng = np.random.default_rng(nc * 100 + n_keys)
    seen = np.zeros(4, np.int32)
    for trial in range(300):
        n = int(rng.integers(1, 120))
        ops = np.zeros((n, 5), np.int32)
        split = int(rng.integers(1, nc))  # the cameras of the first key frame, as the walk pairs them
        across = rng.random() < 0.7
        for k in range(n):
            if across:
                ci, cj = rng.integers(0, split), rng.integers(split, nc)
            else:  # any two cameras, as FillMatchesFromPair allows
                ci, cj = rng.choice(nc, 2, replace=False)
            ops[k] = ci, rng.integers(n_keys), cj, rng.integers(n_keys), rng.integers(0, 8) * 7
        assert lib().tw_fill_compare(nc, n_keys, p(ops), n, p(seen)) == -1, (trial, ops.tolist())
    print("two groups %d, displaced %d, new group %d, turned away %d" % tuple(seen))
    assert seen[2] > 0 and seen[3] > 0 and (nc == 2 or (seen[0] > 100 and seen[1] > 100))


def test_plan_offsets_of_rig_key_frames_with_groups():
    """GetMapn2idxs / v3dpoints_ of rig key frames: the group counts come out of the entry's check (largest group index + 1)
    and the plan's group offsets are their running sum; a group index below -1, or groups without their points, fail"""
    from tests.test_new_points import make_rig_stereo_case
    kf1, st1, kf2s, st2s = make_rig_stereo_case()[:4]
    sts = [st1] + st2s
    counts = [int(s.key_group.max()) + 1 for s in sts]
    assert min(counts) > 5 and all(len(s.group_p3d) == c for s, c in zip(sts, counts))
    P = plan(kf1, kf2s, stereo=(st1, st2s))
    assert P.rc > 0 and P.offs[3].tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    assert P.offs[0].tolist() == np.concatenate([[0], np.cumsum([len(k.keys) for k in [kf1] + kf2s])]).tolist()
    assert not plan(kf1, kf2s).offs[3].any()  # the search alone has no stereo records
    st2s[1].rec[0]["group_p3d"] = 0
    assert plan(kf1, kf2s, stereo=(st1, st2s)).rc == VIEO_E_INVALID
    assert lib().tw_error() == b"CreateNewMapPoints: neighbour 1 is inconsistent"
    st2s[1].rec[0]["group_p3d"] = st2s[1].group_p3d.ctypes.data
    st1.key_group[3] = -2
    assert plan(kf1, kf2s, stereo=(st1, st2s)).rc == VIEO_E_INVALID and lib().tw_error() == b"CreateNewMapPoints: pKF1 is inconsistent"
    st1.key_group[3] = -1
    assert plan(kf1, kf2s, stereo=(st1, st2s)).rc > 0


def test_every_situation_of_the_walk_occurred(oracle):
    """the situations the walk decides on, each met by a case above (this test runs them if it is run alone)"""
    if not _events:
        for name in SCENES:
            test_plan_and_walk_against_the_oracle(oracle, name)
        test_planted_tie_goes_to_the_later_key(oracle)
        test_planted_displacement_on_a_rig(oracle)
    seen = collections.Counter()
    for (name, k), v in _events.items():
        seen[k] += v
        if name in ("radtan", "kb8"):
            seen["rig: " + k] += v
    for k in ("tie", "taken", "displaced", "rotation", "one member", "rig: contradiction, the other group wins",
              "rig: contradiction, the first group wins", "rig: second image"):
        assert seen[k] > 0, (k, dict(seen))


# ---------------------------------------------------------------------------------------------------------------------
def stereo_of(kf1, kf2s):
    return TriStereo(kf1, BF), [TriStereo(k, BF) for k in kf2s]


def test_a_skipped_neighbour_between_two_searched_ones(oracle):
    kf1, kf2s, _ = tri_search.make_tri_scene(27, n_points=400, n_neighbours=3)
    st1, st2s = stereo_of(kf1, kf2s)
    st2s[1] = TriStereo(kf2s[1], BF, Ow=st1.Ow + f32(0.01))  # 1.7 cm from pKF1, its stereo baseline is 10 cm
    assert [new_points_ref.baseline_short(st1, s) for s in st2s] == [False, True, False]
    P = plan(kf1, kf2s, stereo=(st1, st2s))
    assert [tuple(r) for r in P.queries[:, :4].tolist()] == expected_queries(kf1, kf2s, False, skipped=(1,))
    assert P.q_begin[1] == P.q_begin[2] and 0 < P.q_begin[1] < P.q_begin[3] == len(P.queries)
    assert plan(kf1, kf2s).q_begin[2] > P.q_begin[2]  # the search alone does not skip
    P = plan(kf1, kf2s, stereo=(st1, st2s))
    cand, cand_n = gates_table(oracle, kf1, kf2s, P, False)
    rc, pairs, n_pairs, n_matches = walk(kf1, kf2s, cand, cand_n)
    ref = oracle.search_for_triangulation(kf1, kf2s)
    assert rc == VIEO_OK and n_pairs[1] == 0 and n_matches[1] == 0 and (pairs[1] == 7).all()
    for pr in (0, 2):
        assert n_matches[pr] == ref[pr][1] and np.array_equal(pairs[pr, :n_pairs[pr], :2], ref[pr][0]) and len(ref[pr][0]) > 20


def test_capacity_writes_what_fits_and_counts_all(oracle):
    kf1, kf2s, _ = tri_search.make_tri_scene(28, n_points=400, n_neighbours=3)
    order = np.argsort([len(r[0]) for r in oracle.search_for_triangulation(kf1, kf2s)])
    kf2s = [kf2s[order[0]], kf2s[order[2]], kf2s[order[1]]]  # the one with the most rows in the middle
    P = plan(kf1, kf2s)
    cand, cand_n = gates_table(oracle, kf1, kf2s, P, False)
    ref = oracle.search_for_triangulation(kf1, kf2s)
    counts = [len(r[0]) for r in ref]
    cap = counts[1] - 3
    assert counts[0] <= cap < counts[1]  # the first neighbour fits, the second does not
    rc, pairs, n_pairs, n_matches = walk(kf1, kf2s, cand, cand_n, cap=cap)
    assert rc == VIEO_E_CAPACITY
    assert lib().tw_error() == b"SearchForTriangulation: neighbour 1 has %d matches, capacity %d" % (counts[1], cap)
    assert n_pairs[:2].tolist() == counts[:2] and n_matches[:2].tolist() == [r[1] for r in ref[:2]]
    assert np.array_equal(pairs[0, :counts[0]], ref[0][0]) and np.array_equal(pairs[1], ref[1][0][:cap])
    assert (pairs[2:] == 7).all() and n_pairs[2] == -5  # nothing behind the neighbour's block; the call ends there
    rc, pairs, n_pairs, _ = walk(kf1, kf2s, cand, cand_n, cap=0)
    assert rc == VIEO_E_CAPACITY and n_pairs[0] == counts[0]


def test_walk_reports_key_angles_outside_the_histogram(oracle):
    kf1, kf2s, _ = tri_search.make_tri_scene(28, n_points=400, n_neighbours=2)
    P = plan(kf1, kf2s)
    cand, cand_n = gates_table(oracle, kf1, kf2s, P, False)
    kf1.keys["angle"] = 1000.0
    assert walk(kf1, kf2s, cand, cand_n, check=False)[0] == VIEO_OK
    assert walk(kf1, kf2s, cand, cand_n, check=True)[0] == VIEO_E_INVALID
    assert lib().tw_error() == b"SearchForTriangulation: key angles outside [0, 360)"


def test_checks_keep_each_entry_s_texts():
    kf1, kf2s, _ = tri_search.make_tri_scene(29, n_points=100, n_neighbours=2)
    rig1, rig2s, _ = tri_search.make_tri_scene(29, n_points=100, n_neighbours=1, rig="radtan")
    st1, st2s = stereo_of(kf1, kf2s)
    bad = rebuilt(kf1, feat_vec=[(5, [0]), (3, [1])])  # nodes not ascending
    for stereo, who in ((None, b"SearchForTriangulation"), ((st1, st2s), b"CreateNewMapPoints")):
        assert plan(kf1, kf2s, stereo=stereo).rc > 0
        assert plan(bad, kf2s, stereo=stereo).rc == VIEO_E_INVALID
        tail = b" (nodes ascending, feature / camera indices and octaves in range)" if stereo is None else b""
        assert lib().tw_error() == who + b": pKF1 is inconsistent" + tail
        assert plan(kf1, [kf2s[0], bad], stereo=stereo).rc == VIEO_E_INVALID
        assert lib().tw_error() == who + b": neighbour 1 is inconsistent"
        assert plan(kf1, kf2s, stereo=stereo, stride=1).rc == VIEO_E_INVALID
        assert lib().tw_error() == who + b": pair_stride 1 is smaller than the cameras of pair 0"
    assert plan(rig1, kf2s, stride=8).rc == VIEO_E_INVALID
    assert lib().tw_error() == b"SearchForTriangulation: neighbour 0 and pKF1 are not of one kind (undistorted / rig)"
    nodepth = TriStereo(kf2s[1], BF)
    nodepth.rec[0]["depth"] = 0
    assert plan(kf1, kf2s, stereo=(st1, [st2s[0], nodepth])).rc == VIEO_E_INVALID
    assert lib().tw_error() == b"CreateNewMapPoints: neighbour 1 is inconsistent"


# ---------------------------------------------------------------------------------------------------------------------
# the gather and the scatter of the triangulation
def gather(kf1, st1, kf2s, st2s, rows, cap=None, n_pairs=None):
    n = len(kf2s)
    cap = int(cap if cap is not None else max(len(r) for r in rows))
    stride = stride_of(kf1, kf2s) + 1  # one column of padding
    pairs = np.full((n, cap, stride), 7, np.int32)
    for pr, r in enumerate(rows):
        pairs[pr, :min(len(r), cap), :r.shape[1]] = r[:cap]
    n_pairs = np.array([len(r) for r in rows] if n_pairs is None else n_pairs, np.int32)
    out = dict(status=np.full((n, cap), 99, np.int8), x3d=np.full((n, cap, 3), 5.0), x3d_f=np.full((n, cap, 3), 5.0, f32),
               n_new=np.full(n, 99, np.int32))
    g_rows, g_pair, g_dst = np.full((n * cap + 1, stride), 9, np.int32), np.zeros(n * cap + 1, np.int32), np.zeros(n * cap + 1, np.int64)
    rc = lib().tw_gather(p(kf1.rec), p(st1.rec), p(recs(kf2s)), p(recs(st2s)), n, cap, stride, p(pairs), p(n_pairs), p(out["status"]),
                         p(out["x3d"]), p(out["x3d_f"]), p(out["n_new"]), p(g_rows), p(g_pair), p(g_dst))
    return rc, out, g_rows[:max(rc, 0)], g_pair[:max(rc, 0)], g_dst[:max(rc, 0)], pairs, cap


@pytest.mark.parametrize("rig", [None, "radtan"])
def test_gather_and_scatter(oracle, rig):
    kf1, kf2s, _ = tri_search.make_tri_scene(30, n_points=400, n_neighbours=3, rig=rig)
    st1, st2s = stereo_of(kf1, kf2s)
    st2s[1] = TriStereo(kf2s[1], BF, Ow=st1.Ow + f32(0.01))
    rows = [r[0] for r in oracle.search_for_triangulation(kf1, kf2s)]
    counts = [len(r) for r in rows]
    assert min(counts) > 20
    rc, out, g_rows, g_pair, g_dst, pairs, cap = gather(kf1, st1, kf2s, st2s, rows)
    # the short-baseline neighbour: SKIPPED rows with zeroed points, none of them gathered
    assert rc == counts[0] + counts[2] and g_pair.tolist() == [0] * counts[0] + [2] * counts[2]
    assert (out["status"][1, :counts[1]] == NEWPT_SKIPPED).all() and not out["x3d"][1, :counts[1]].any() and not out["x3d_f"][1, :counts[1]].any()
    assert (out["status"][1, counts[1]:] == 99).all() and (out["status"][[0, 2]] == 99).all() and (out["x3d"][[0, 2]] == 5).all()
    assert out["n_new"].tolist() == [0, 0, 0]
    assert g_dst.tolist() == list(range(counts[0])) + [2 * cap + m for m in range(counts[2])]
    for pr in (0, 2):  # the rows as given, every column past the pair's cameras -1
        nc = kf1.n_cams + kf2s[pr].n_cams
        assert np.array_equal(g_rows[g_pair == pr][:, :nc], rows[pr]) and (g_rows[g_pair == pr][:, nc:] == -1).all()
    # the scatter: results to row_dst, accepted rows counted per neighbour
    rng = np.random.default_rng(1)
    st = rng.integers(-7, 3, rc).astype(np.int8)
    x3d, x3d_f = rng.normal(size=(rc, 3)), rng.normal(size=(rc, 3)).astype(f32)
    lib().tw_scatter(3, cap, p(st), p(x3d), p(x3d_f), p(out["status"]), p(out["x3d"]), p(out["x3d_f"]), p(out["n_new"]))
    flat = lambda a: a.reshape((3 * cap,) + a.shape[2:])
    assert np.array_equal(flat(out["status"])[g_dst], st) and np.array_equal(flat(out["x3d"])[g_dst], x3d)
    assert np.array_equal(flat(out["x3d_f"])[g_dst], x3d_f)
    assert out["n_new"].tolist() == [int((st[g_pair == pr] >= 0).sum()) for pr in range(3)] and out["n_new"][1] == 0
    untouched = np.ones(3 * cap, bool)
    untouched[g_dst] = False
    untouched[cap:cap + counts[1]] = False
    assert (flat(out["status"])[untouched] == 99).all() and (flat(out["x3d"])[untouched] == 5).all()
    # the errors
    rc = gather(kf1, st1, kf2s, st2s, rows, n_pairs=[counts[0], counts[1], -1])[0]
    assert rc == VIEO_E_INVALID and lib().tw_error() == b"CreateNewMapPoints: neighbour 2 has a negative row count"
    rc = gather(kf1, st1, kf2s, st2s, rows, cap=counts[0] - 1)[0]
    assert rc == VIEO_E_CAPACITY
    assert lib().tw_error() == b"CreateNewMapPoints: neighbour 0 has %d rows, capacity %d" % (counts[0], counts[0] - 1)
    nc1 = kf1.n_cams
    c1 = int(np.flatnonzero(rows[2][4][:nc1] >= 0)[0])
    c2 = nc1 + int(np.flatnonzero(rows[2][4][nc1:] >= 0)[0])
    for col, key in ((c1, len(kf1.keys)), (c2, len(kf2s[2].keys)), (c1, -2), (c2, -2)):
        wrong = [r.copy() for r in rows]
        wrong[2][4, col] = key
        assert gather(kf1, st1, kf2s, st2s, wrong)[0] == VIEO_E_INVALID
        assert lib().tw_error() == b"CreateNewMapPoints: row 4 of neighbour 2 holds key %d" % key
    wrong = [r.copy() for r in rows]
    wrong[1][4, c1] = len(kf1.keys)  # (the rows of a skipped neighbour are not looked at)
    assert gather(kf1, st1, kf2s, st2s, wrong)[0] == counts[0] + counts[2]
