"""The two projection searches of a loop closure that take a Sim3 world pose: ORBmatcher::SearchByProjection(KeyFrame*,
Scw, ...) (vieo_search_by_projection_scw) and ORBmatcher::Fuse(KeyFrame*, Scw, ...) for every key frame of a SearchAndFuse
in one call (vieo_fuse_scw), against the restatement of tests/loop_close_ref.py.

The CPU tests come first and check the restatement and the scenes, so neither certifies itself: Fuse's projection stage
against the oracle's vo_fuse_search with the viewing cone on, SearchByProjection as the reference writes it (vpMatched
consulted inside the candidate loop) against a second statement that lists and replays, on the scenes and on random
candidate tables, and every situation the scenes plant.  The GPU tests ask every output byte for byte."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from tests import loop_close_ref as ref
from tests import loop_verify_ref as vref
from vieo_slam_amd import _lib
from vieo_slam_amd import loop_closing as lc

KINDS = ["one", "rig"]


@functools.lru_cache(maxsize=None)
def _scene(kind):
    if kind == "one":
        return lc.make_loop_close_scene(21)
    return lc.make_loop_close_scene(22, n_cams=2)


@functools.lru_cache(maxsize=None)
def _search(kind):
    """the restatement of SearchByProjection on a scene, once: (matched, nmatches, lists)"""
    s = _scene(kind)
    m, n = ref.search_by_projection_scw(s["kf1"], s["Scw"], s["points"], s["ids"], s["matched"])
    return m, n, ref.scw_lists(s["kf1"], s["Scw"], s["points"], s["ids"], s["matched"])


@functools.lru_cache(maxsize=None)
def _fuse_visits(kind):
    """[(key frame index, Scw)]: the corrected key frames of the scene, and the current one again through candidate 1"""
    s = _scene(kind)
    visits = [(i, S) for i, S in enumerate(s["fuse_Scws"])]
    return visits + [(0, lc.sim3_world_pose(s["kf2s"][1], *s["sim3"][1])[3])]


@functools.lru_cache(maxsize=None)
def _fused(kind):
    """the restatement of Fuse on every visit of a scene, once"""
    s = _scene(kind)
    return [ref.fuse_scw(s["fuse_kfs"][k], S, s["points"], s["ids"], detail=True) for k, S in _fuse_visits(kind)]


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the restatement
@pytest.mark.parametrize("kind", KINDS)
def test_restated_fuse_projection_stage_against_the_oracle(oracle, kind):
    s = _scene(kind)
    for (k, _), o in zip(_fuse_visits(kind), _fused(kind)):
        kf = s["fuse_kfs"][k]
        bi, bd = ref.oracle_project_stage(oracle, kf, *o["transform"], lc.TH_SCW_FUSE, s["points"], s["ids"], o["mask"])
        assert (bi >= 0).sum() > 60
        assert np.array_equal(bi, o["best_idx"]) and np.array_equal(bd, o["best_dist"])


def test_restated_decompositions_are_the_pose_of_the_sim3():
    s = _scene("one")
    sc, R, t, Scw = lc.sim3_world_pose(s["kf2s"][0], *s["sim3"][0])
    Re, te, twcr = ref.decompose_eigen(Scw)
    Rc, tc = ref.decompose_cv(Scw)
    for Rx, tx in ((Re, te), (Rc, tc)):
        assert np.abs(Rx - R).max() < 1e-6 and np.abs(tx - t / sc).max() < 1e-5
    assert np.abs(twcr + R.T @ t / sc).max() < 1e-5
    # the two decompositions are different arithmetic: close, and on these scenes not equal in every bit
    assert np.abs(Re - Rc).max() < 2e-7


@pytest.mark.parametrize("kind", KINDS)
def test_restated_search_against_list_and_replay(kind):
    s = _scene(kind)
    m, n, lists = _search(kind)
    m2, n2 = ref.replay_lists(lists, s["ids"], s["matched"])
    assert np.array_equal(m, m2) and n == n2
    assert n >= lc.LOOP_MATCHES  # the scene adds matches
    assert (s["matched"] >= 0).sum() >= 30 and np.array_equal(m[s["matched"] >= 0], s["matched"][s["matched"] >= 0])
    # a point that was already found is not searched, nor is a bad one
    found = set(int(i) for i in s["matched"] if i >= 0)
    assert all(not any(lists[i]) for i in range(len(s["ids"])) if int(s["ids"][i]) in found)


def test_restated_search_on_random_candidate_tables():
    """random windows of few keys, so that keys are contested: the statement with vpMatched inside the candidate loop and
    the list-and-replay one must agree on who gets which key"""
    rng = np.random.default_rng(9)
    contested = 0
    for _ in range(30):
        n_keys, n_points, nc = 12, 25, 2
        lists = []
        for _ in range(n_points):
            per_cam = []
            for c in range(nc):
                keys = rng.choice(n_keys // nc, rng.integers(0, 4), replace=False) * nc + c
                per_cam.append([(int(k), int(rng.integers(40, 52)), pos) for pos, k in enumerate(keys)])
            lists.append(per_cam)
        ids = np.arange(100, 100 + n_points)
        matched0 = np.where(rng.uniform(size=n_keys) < 0.2, 7, -1).astype(np.int32)
        # the reference's structure on the same tables
        matched, n = matched0.copy(), 0
        for iMP in range(n_points):
            for c in range(nc):
                bestDist, bestIdx = 256, -1
                for idx, dist, _ in lists[iMP][c]:
                    if matched[idx] >= 0:
                        continue
                    if dist < bestDist:
                        bestDist, bestIdx = dist, idx
                if bestDist <= ref.TH_LOW:
                    matched[bestIdx] = ids[iMP]
                    n += 1
        listed = [[[e for e in cands if e[1] <= ref.TH_LOW] for cands in per_cam] for per_cam in lists]
        m2, n2 = ref.replay_lists(listed, ids, matched0)
        assert np.array_equal(matched, m2) and n == n2
        contested += sum(1 for per_cam in listed for cands in per_cam if cands and all(matched0[k] >= 0 or m2[k] != -1 for k, _, _ in cands))
    assert contested > 100


@pytest.mark.parametrize("kind", KINDS)
def test_search_scene_holds_what_it_plants(kind):
    s = _scene(kind)
    kf, ids, pl = s["kf1"], s["ids"], s["planted"]
    m, _, lists = _search(kind)
    holder = lambda i: [int(k) for k in np.flatnonzero(m == ids[i])]
    # a key taken by an earlier point: the later point takes its second best; the third finds every candidate taken
    a, b, c = pl["taken"]["points"]
    k1, k2 = pl["taken"]["keys"]
    assert [e[:2] for e in lists[a][0]] == [e[:2] for e in lists[b][0]] == [e[:2] for e in lists[c][0]] == [(k1, 5), (k2, 20)]
    assert holder(a) == [k1] and holder(b) == [k2] and holder(c) == []
    # two candidates at equal distance: the earlier one in the candidate order
    (ka, da, pa), (kb, db, pb) = lists[pl["tie"]["point"]][0]
    assert da == db == 7 and pa < pb and holder(pl["tie"]["point"]) == [ka] and {ka, kb} == set(pl["tie"]["keys"])
    # distances 50 and 51: the second key is in its point's window and only its distance keeps it out
    p50, p51 = pl["edge"]["points"]
    k50, k51 = pl["edge"]["keys"]
    assert [e[:2] for e in lists[p50][0]] == [(k50, 50)] and holder(p50) == [k50]
    assert lists[p51][0] == [] and holder(p51) == []
    R, t, twcr = ref.decompose_eigen(s["Scw"])
    u, v, lvl, radius = ref._project(kf, R, t, twcr, s["points"][p51], 0, lc.TH_SCW_SEARCH)
    grids = [vref.build_grid(kf, c_) for c_ in range(kf.n_cams)]
    assert k51 in [k for _, k in ref._window(kf, grids, 0, u, v, radius)]
    assert ref._hamming(s["points"][p51]["desc"], kf.desc[k51]) == 51 and lvl - 1 <= kf.keys[k51]["octave"] <= lvl
    # more than 64 keys in one column run of the window, all of them candidates
    crowd = pl["crowd"]
    assert len(lists[crowd["point"]][0]) == 70 and set(k for k, _, _ in lists[crowd["point"]][0]) == set(crowd["keys"])
    cols = {}
    for (ix, iy), ks in grids[0].items():
        cols[ix] = cols.get(ix, 0) + len(set(ks) & set(crowd["keys"]))
    assert max(cols.values()) > 64
    pos = [p for _, _, p in lists[crowd["point"]][0]]
    assert pos == sorted(pos) and len(set(pos)) == 70
    # the viewing cone: 0.1 per mille inside matches, 0.1 per mille outside is not searched -- and would match without it
    inside, outside = pl["cone"]["points"]
    assert holder(inside) == [pl["cone"]["keys"][0]] and lists[outside][0] == []
    no_cone = ref.scw_lists(kf, s["Scw"], s["points"][outside:outside + 1], ids[outside:outside + 1], s["matched"], cone=False)
    assert [e[:2] for e in no_cone[0][0]] == [(pl["cone"]["keys"][1], 3)]
    if kind == "rig":  # a point matched in both cameras
        both = [i for i in range(len(ids)) if sorted(int(kf.cam_of_key[k]) for k in holder(i)) == [0, 1]]
        assert len(both) >= 10


@pytest.mark.parametrize("kind", KINDS)
def test_fuse_scene_holds_what_it_plants(kind):
    s = _scene(kind)
    ids = s["ids"]
    where = {int(i): m for m, i in enumerate(ids)}
    same_key = two_keys = masked_low = masked_high = other_cam = 0
    for (k, _), o in zip(_fuse_visits(kind), _fused(kind)):
        kf = s["fuse_kfs"][k]
        assert o["n_fused"] >= 60 and (o["replace"] >= 0).sum() >= 10 and o["added"].sum() >= 10
        assert o["n_fused"] == sum(len(x) for x in o["sets"])
        # two loop points on the same free key: the first is added, the second gets the first as its replace
        for m2 in np.flatnonzero(o["replace"] >= 0):
            m1 = where.get(int(o["replace"][m2]))
            if m1 is not None and m1 < m2 and o["added"][m1].any() and set(o["sets"][m1]) & set(o["sets"][m2]):
                same_key += 1
        # a set with two keys that hold different points: the larger key decides
        for m, keys in enumerate(o["sets"]):
            if len(keys) != 2 or o["added"][m].any():
                continue
            id0, id1 = int(kf.mp_id[keys[0]]), int(kf.mp_id[keys[1]])
            if id0 >= 0 and id1 >= 0 and id0 != id1:
                assert keys[0] < keys[1] and o["replace"][m] == id1
                two_keys += 1
        # the mask as written: the camera of KEY index iMP
        n = len(kf.keys)
        holders = {}
        for key, (i, c) in enumerate(zip(kf.mp_id, kf.cam_of_key)):
            if i >= 0:
                holders.setdefault(int(i), set()).add(int(c))
        for m in range(len(ids)):
            cams = holders.get(int(ids[m]), set())
            cam = int(kf.cam_of_key[m]) if m < n else 0
            assert (o["mask"][m] != 0) == (cam in cams) and o["mask"][m] in (0, 1 << cam)
            if o["mask"][m]:
                masked_low += m < n
                masked_high += m >= n
                assert o["best_idx"][m, cam] == -1
            elif cams:
                other_cam += 1
    assert same_key >= 3 and masked_low >= 20
    if kind == "one":
        assert masked_high >= 10  # the table is longer than a key frame's keys
    else:
        assert two_keys >= 1 and other_cam >= 5 and s["planted"]["two_ids"]


# ---------------------------------------------------------------------------------------------------------------------
# GPU
def _lists_equal(got, want):
    return len(got) == len(want) and all(g == w for g, w in zip(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_search_by_projection_scw_equals_the_restatement(kind):
    s = _scene(kind)
    m, n, lists = _search(kind)
    (gm, gn), = lc.SearchByProjectionScw([s["kf1"]], s["points"], s["ids"], [(0, s["Scw"], s["matched"])])
    tap = lc.search_by_projection_scw_tap(len(s["ids"]), s["kf1"].n_cams, 0)
    assert _lists_equal(tap, lists)
    assert gn == n and gm.tobytes() == m.tobytes()
    items, survivors = lc.scw_gate_stats()
    assert items == len(s["ids"]) * s["kf1"].n_cams and 0 < survivors < items


@pytest.mark.gpu
def test_search_by_projection_scw_visits_in_one_call_and_a_small_pool(monkeypatch):
    """two visits of the current key frame (another Sim3, another vpMatched) and one of a candidate in one call equal the
    restatement of each; a pool of 16 entries makes the call list again into an exact one, with the same bytes"""
    s = _scene("one")
    kfs = [s["kf1"], s["fuse_kfs"][1]]
    Scw2 = lc.sim3_world_pose(s["kf2s"][1], *s["sim3"][1])[3]
    m2 = s["matched"].copy()
    m2[::2] = -1
    m3 = np.full(len(kfs[1].keys), -1, np.int32)
    visits = [(0, s["Scw"], s["matched"]), (0, Scw2, m2), (1, s["fuse_Scws"][1], m3)]
    want = [ref.search_by_projection_scw(kfs[k], S, s["points"], s["ids"], m) for k, S, m in visits]
    assert all(n >= 40 for _, n in want)
    first = lc.SearchByProjectionScw(kfs, s["points"], s["ids"], visits)
    taps = [lc.search_by_projection_scw_tap(len(s["ids"]), 1, v) for v in range(3)]
    monkeypatch.setenv("VIEO_SCW_POOL", "16")
    small = lc.SearchByProjectionScw(kfs, s["points"], s["ids"], visits)
    for v, ((wm, wn), (gm, gn), (sm, sn)) in enumerate(zip(want, first, small)):
        assert gn == wn == sn and gm.tobytes() == wm.tobytes() == sm.tobytes()
        assert _lists_equal(lc.search_by_projection_scw_tap(len(s["ids"]), 1, v), taps[v])
        assert _lists_equal(taps[v], ref.scw_lists(kfs[visits[v][0]], visits[v][1], s["points"], s["ids"], visits[v][2]))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_fuse_scw_equals_the_restatement_visit_by_visit(kind):
    s = _scene(kind)
    nc = s["kf1"].n_cams
    for (k, S), o in zip(_fuse_visits(kind), _fused(kind)):
        g, = lc.FuseScw(s["fuse_kfs"], s["points"], s["ids"], [(k, S)])
        bi, bd = lc.fuse_scw_tap(len(s["ids"]), nc, 0)
        assert np.array_equal(bi, o["best_idx"]) and np.array_equal(bd, o["best_dist"])
        assert g["n_fused"] == o["n_fused"]
        for name in ("match_key", "replace", "added"):
            assert g[name].tobytes() == o[name].tobytes(), name


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_fuse_scw_four_visits_equal_four_calls_and_a_second_call(kind):
    """the order in which the gate compacts its survivors must not show"""
    s = _scene(kind)
    visits = _fuse_visits(kind)
    assert len(visits) == 4
    singles = [lc.FuseScw(s["fuse_kfs"], s["points"], s["ids"], [v])[0] for v in visits]
    one = lc.FuseScw(s["fuse_kfs"], s["points"], s["ids"], visits)
    items, survivors = lc.scw_gate_stats()
    assert items == 4 * len(s["ids"]) * s["kf1"].n_cams and 0 < survivors < items
    two = lc.FuseScw(s["fuse_kfs"], s["points"], s["ids"], visits)
    for a, b, c, o in zip(singles, one, two, _fused(kind)):
        assert a["n_fused"] == b["n_fused"] == c["n_fused"] == o["n_fused"]
        for name in ("match_key", "replace", "added"):
            assert a[name].tobytes() == b[name].tobytes() == c[name].tobytes() == o[name].tobytes(), name
    res = lc.SearchAndFuse([s["fuse_kfs"][k] for k, _ in visits[:3]], [S for _, S in visits[:3]], s["points"], s["ids"])
    for r, o in zip(res, _fused(kind)):
        assert r["n_fused"] == o["n_fused"] and all(o["match_key"][m].tolist().count(k) == 1 for m, k in r["add"])
        assert len(r["add"]) == o["added"].sum() and [m for _, m in r["replace"]] == [int(m) for m in np.flatnonzero(o["replace"] >= 0)]


@functools.lru_cache(maxsize=None)
def _shape_scenes():
    """small scenes of different shape: a 4-camera pair scene, the loop closure on top of the same pair (make_loop_close_scene
    starts from make_loop_pair_scene with its arguments), and a 1-camera loop closure with a fifth of the keys"""
    pair = lc.make_loop_pair_scene(31, n_keys=200, n_points=30, n_cams=4, n_cands=2)
    return pair, lc.make_loop_close_scene(31, n_keys=200, n_points=30, n_cams=4), lc.make_loop_close_scene(32, n_keys=40, n_points=30)


@functools.lru_cache(maxsize=None)
def _shape_restated():
    """the restatements of the calls of test_one_staging_serves_calls_of_changing_shape, once"""
    pair, rig, one = _shape_scenes()
    entry = np.full(len(pair["kf1"].keys), -1, np.int32)
    sim3 = vref.search_by_sim3(pair["kf1"], pair["kf2s"][0], *pair["sim3"][0], entry, detail=True)
    search = ref.search_by_projection_scw(one["kf1"], one["Scw"], one["points"], one["ids"], one["matched"])
    lists = ref.scw_lists(one["kf1"], one["Scw"], one["points"], one["ids"], one["matched"])
    fuse = [ref.fuse_scw(rig["fuse_kfs"][k], S, rig["points"], rig["ids"], detail=True) for k, S in enumerate(rig["fuse_Scws"])]
    return sim3, search, lists, fuse


def test_shape_scenes_differ_in_every_stride():
    pair, rig, one = _shape_scenes()
    sim3, search, lists, fuse = _shape_restated()
    assert pair["kf1"].n_cams == rig["kf1"].n_cams == 4 and one["kf1"].n_cams == 1
    assert len(one["kf1"].keys) < len(pair["kf1"].keys) < len(rig["fuse_kfs"][0].keys)  # key_cap of the three stagings
    assert len(set(pair["kf1"].cam_of_key.tolist())) == 4  # the permutation into camera order is not the identity
    assert (np.diff(pair["kf1"].cam_of_key) < 0).any()
    # and every call finds something to get wrong
    assert sim3[1] >= 5 and all((d[0] >= 0).sum() >= 10 for d in (sim3[2]["fwd"], sim3[2]["bwd"]))
    assert search[1] >= 10 and sum(1 for per_cam in lists if any(per_cam)) >= 10
    assert all(o["n_fused"] >= 10 and (o["best_idx"] >= 0).sum() >= 10 for o in fuse)


@pytest.mark.gpu
def test_one_staging_serves_calls_of_changing_shape():
    """The map-side calls share one staging object per thread.  Calls of different shape in one process -- 4 cameras and 200
    keys per slot with the points beside them, 1 camera and fewer keys, 4 cameras and more keys, the per-camera arrays of one
    frame, the first again -- must each equal their restatement: a stride kept from the call before would move every slot
    but the first."""
    from vieo_slam_amd import map_point as mp
    pair, rig, one = _shape_scenes()
    w_sim3, w_search, w_lists, w_fuse = _shape_restated()
    visit = (0,) + tuple(pair["sim3"][0]) + (np.full(len(pair["kf1"].keys), -1, np.int32),)

    def sim3():
        (m, n), = lc.SearchBySim3(pair["kf1"], pair["kf2s"], [visit])
        return [m, n] + [a for d in (0, 1) for a in lc.search_by_sim3_tap(pair["kf1"], pair["kf2s"][0], 0, d)]

    first = sim3()
    assert first[0].tobytes() == w_sim3[0].tobytes() and first[1] == w_sim3[1]
    for got, want in zip(first[2:], [w_sim3[2][d][i] for d in ("fwd", "bwd") for i in (0, 1)]):
        assert np.array_equal(got, want)
    (gm, gn), = lc.SearchByProjectionScw([one["kf1"]], one["points"], one["ids"], [(0, one["Scw"], one["matched"])])
    assert _lists_equal(lc.search_by_projection_scw_tap(len(one["ids"]), 1, 0), w_lists)
    assert gn == w_search[1] and gm.tobytes() == w_search[0].tobytes()
    visits = list(enumerate(rig["fuse_Scws"]))
    fused = lc.FuseScw(rig["fuse_kfs"], rig["points"], rig["ids"], visits)
    taps = [lc.fuse_scw_tap(len(rig["ids"]), 4, v) for v in range(len(visits))]
    for g, (bi, bd), o in zip(fused, taps, w_fuse):
        assert np.array_equal(bi, o["best_idx"]) and np.array_equal(bd, o["best_dist"])
        assert g["n_fused"] == o["n_fused"]
        for name in ("match_key", "replace", "added"):
            assert g[name].tobytes() == o[name].tobytes(), name
    # vieo_fuse_search on the last key frame with the same transform and masks (the module stands in for the oracle)
    k, o = len(visits) - 1, w_fuse[-1]
    bi, bd = ref.oracle_project_stage(mp, rig["fuse_kfs"][k], *o["transform"], lc.TH_SCW_FUSE, rig["points"], rig["ids"], o["mask"])
    assert np.array_equal(bi, taps[k][0]) and np.array_equal(bd, taps[k][1])
    again = sim3()
    assert first[1] == again[1] and all(a.tobytes() == b.tobytes() for a, b in zip(first[:1] + first[2:], again[:1] + again[2:]))


def _with_rec(kf, **fields):
    """the key frame with fields of its record replaced (the arrays stay kf's)"""
    rec = kf.rec.copy()
    for name, value in fields.items():
        rec[name] = value
    return SimpleNamespace(rec=rec, n_cams=kf.n_cams, keys=kf.keys)


def _refusals(s):
    """name -> (kfs, visit key frame, null point table, th) of every call that must be refused"""
    kfs = s["fuse_kfs"][:2]
    keys = kfs[1].keys.copy()
    keys["octave"][5] = 8
    bounds = kfs[1].rec["bounds"].copy()
    bounds[0, 0, 1] += 1.0
    return {"key frame outside the table": (kfs, 2, False, 4.0),
            "17 levels": ([kfs[0], _with_rec(kfs[1], n_levels=17)], 0, False, 4.0),
            "differing bounds": ([kfs[0], _with_rec(kfs[1], bounds=bounds)], 0, False, 4.0),
            "octave out of range": ([kfs[0], lc._copy_kf(kfs[1], keys=keys)], 0, False, 4.0),
            "null point table": (kfs, 0, True, 4.0),
            "th = 0": (kfs, 0, False, 0.0)}


@pytest.mark.gpu
def test_refused_arguments_touch_nothing():
    s = _scene("one")
    L = _lib.lib()
    n = len(s["ids"])
    good_kfs = s["fuse_kfs"][:2]
    # a good call of either entry first: its tap must survive every refusal
    lc.SearchByProjectionScw(good_kfs, s["points"], s["ids"], [(0, s["Scw"], s["matched"][:len(good_kfs[0].keys)])])
    lc.FuseScw(good_kfs, s["points"], s["ids"], [(0, s["Scw"])])
    tap_a, tap_b = lc.search_by_projection_scw_tap(n, 1, 0), lc.fuse_scw_tap(n, 1, 0)
    pts, ids = np.ascontiguousarray(s["points"]), np.ascontiguousarray(s["ids"], np.int32)
    for name, (kfs, kf, null_table, th) in _refusals(s).items():
        recs = np.concatenate([k.rec for k in kfs])
        matched = np.full(len(kfs[min(kf, 1)].keys), -1, np.int32)
        matched[3] = 12345
        before = matched.copy()
        VA = np.zeros(1, lc.SCW_VISIT_DTYPE)
        VA[0]["kf"], VA[0]["Scw"], VA[0]["matched"], VA[0]["n_matches"] = kf, s["Scw"].reshape(-1), matched.ctypes.data, -7
        rc = L.vieo_search_by_projection_scw(recs.ctypes.data, len(kfs), None if null_table else pts.ctypes.data, ids.ctypes.data, n,
                                             VA.ctypes.data, 1, th)
        assert rc == _lib.VIEO_E_INVALID, name
        assert matched.tobytes() == before.tobytes() and VA[0]["n_matches"] == -7, name
        out = [np.full((n, 1), -7, np.int32), np.full(n, -7, np.int32), np.full((n, 1), 7, np.uint8)]
        VB = np.zeros(1, lc.FUSE_SCW_VISIT_DTYPE)
        VB[0]["kf"], VB[0]["Scw"], VB[0]["n_fused"] = kf, s["Scw"].reshape(-1), -7
        VB[0]["match_key"], VB[0]["replace"], VB[0]["added"] = (o.ctypes.data for o in out)
        rc = L.vieo_fuse_scw(recs.ctypes.data, len(kfs), None if null_table else pts.ctypes.data, ids.ctypes.data, n, VB.ctypes.data, 1, th)
        assert rc == _lib.VIEO_E_INVALID, name
        assert (out[0] == -7).all() and (out[1] == -7).all() and (out[2] == 7).all() and VB[0]["n_fused"] == -7, name
        assert _lists_equal(lc.search_by_projection_scw_tap(n, 1, 0), tap_a), name
        bi, bd = lc.fuse_scw_tap(n, 1, 0)
        assert np.array_equal(bi, tap_b[0]) and np.array_equal(bd, tap_b[1]), name
    # the limits: more point-visits than one call takes
    V = np.zeros(5000, lc.FUSE_SCW_VISIT_DTYPE)
    assert L.vieo_fuse_scw(np.concatenate([k.rec for k in good_kfs]).ctypes.data, 2, pts.ctypes.data, ids.ctypes.data, n,
                           V.ctypes.data, 5000, 4.0) == _lib.VIEO_E_CAPACITY


# ---------------------------------------------------------------------------------------------------------------------
# ComputeSim3 as one call (vieo_compute_sim3, loop_closing.ComputeSim3)
N_ROWS = 300


@functools.lru_cache(maxsize=None)
def _c_scene(kind):
    return lc.make_compute_sim3_scene(31) if kind == "match" else lc.make_compute_sim3_scene(32, fail=True)


@functools.lru_cache(maxsize=None)
def _c_samples(kind):
    """the sample tables, one per candidate.  In the matching scene the first five rows of every candidate hold one of
    the outliers SearchByBoW produced (a current key paired with another physical point), so the first pass of the while
    returns no Sim3; the rows behind are drawn as the solver draws."""
    from tests import loop_ref
    s = _c_scene(kind)
    out = []
    for c, kf2 in enumerate(s["kf2s"]):
        m, n, _ = loop_ref.search_by_bow_kf(s["kf1"].bow, kf2.bow, 0.75, True)
        if n < lc.THRESH_MATCHES:
            out.append(np.tile(np.array([0, 1, 2], np.int32), (N_ROWS, 1)))
            continue
        i1 = ref.sim3_candidate(s["kf1"], kf2, m, False)["index1"]
        rows = lc.draw_samples(np.random.default_rng([7, c]), len(i1), N_ROWS)
        if kind == "match":
            wrong = s["kf1"].mp_id[i1] % 1000 != kf2.mp_id[np.asarray(m)[i1]] % 1000
            bad, good = np.flatnonzero(wrong), np.flatnonzero(~wrong)
            assert len(bad) >= 1
            for r in range(5):
                rows[r] = [bad[r % len(bad)], good[2 * r], good[2 * r + 1]]
        out.append(rows)
    return out


@functools.lru_cache(maxsize=None)
def _c_restated(kind):
    s = _c_scene(kind)
    return ref.compute_sim3(s["kf1"], s["kf2s"], lc.THRESH_MATCHES, lc.THRESH_INLIERS, False, _c_samples(kind))


def test_compute_sim3_scenes_hold_what_they_plant():
    o = _c_restated("match")
    assert o["found"] and o["n_inliers"] >= 20 and o["passes"] >= 2
    assert all(line[4] == 0 for line in o["trace"] if line[1] == 1)  # the first pass returns no Sim3
    assert (o["match12"] >= 0).sum() >= 40
    # the Sim3 found is the scene's
    s = _c_scene("match")
    s12, R12, t12 = s["sim3"][o["cand"]]
    assert abs(o["S12"][0] / float(s12) - 1) < 1e-2 and np.abs(o["S12"][1] - R12).max() < 1e-2 and np.abs(o["S12"][2] - t12).max() < 5e-2
    f = _c_restated("fail")
    assert not f["found"] and f["cand"] == -1 and (f["match12"] == -1).all()
    assert f["trace"][0][:4] == (0, 0, -1, 1) and f["trace"][0][5] < lc.THRESH_MATCHES  # discarded by SearchByBoW
    assert f["trace"][1][3] == 0 and f["trace"][1][5] >= lc.THRESH_MATCHES  # kept, then never a Sim3 until bNoMore
    assert f["trace"][-1][0] == 1 and f["trace"][-1][3] == 1 and all(line[4] == 0 for line in f["trace"])


def _mp_compose(S12, kf2):
    """gScm * gSmw with 50 digits: (s R | t) as mpmath numbers"""
    import mpmath as mp
    mp.mp.dps = 50
    s, R12, t12 = mp.mpf(float(S12[0])), mp.matrix(np.asarray(S12[1], np.float64).tolist()), mp.matrix(np.asarray(S12[2], np.float64).tolist())
    R2, t2 = mp.matrix(kf2.Rcw.astype(np.float64).tolist()), mp.matrix(kf2.tcw.astype(np.float64).tolist())
    return s, R12 * R2, s * (R12 * t2) + t12


def _compose_error(s, R, t, exact):
    import mpmath as mp
    es, eR, et = exact
    err = [abs(mp.mpf(float(s)) - es)] + [abs(mp.mpf(float(R[i, j])) - eR[i, j]) for i in range(3) for j in range(3)]
    return float(max(err + [abs(mp.mpf(float(t[i])) - et[i]) for i in range(3)]))


def test_restated_composition_against_50_digits():
    """the numpy composition of Scw against the 50-digit one: the error that sets the bound of the GPU test.
    Measured on the matching scene: 1.1e-16 (half a rounding of an entry of size 1); bound of the GPU test = 8 x that."""
    o = _c_restated("match")
    e = _compose_error(o["s"], o["R"], o["t"], _mp_compose(o["S12"], _c_scene("match")["kf2s"][o["cand"]]))
    print("numpy composition against 50 digits: %.3g" % e)
    assert 0 < e < 1e-15


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["match", "fail"])
def test_compute_sim3_equals_the_restatement(kind):
    """the winner, match12 and every trace line equal the restatement that replays the device's own hypothesis tables (the
    hypotheses themselves are checked in test_loop_sim3.py); Scw within 8 x the numpy composition's own error against the
    50-digit composition of the restatement's S12 and Smw (measured 1.1e-16, so 8.7e-16), mScw its rounding"""
    s = _c_scene(kind)
    smp = _c_samples(kind)
    # the tables of a solver made from the same inputs, for the replay
    want0 = _c_restated(kind)
    kept = sorted(want0["candidates"])
    solver = lc.Sim3Solver([want0["candidates"][c] for c in kept], [smp[c] for c in kept],
                           params=dict(lc.LOOP_SIM3_PARAMS, min_inliers=lc.THRESH_INLIERS))
    tables = {}
    for k, c in enumerate(kept):
        _, sRt, _, mask = solver.rows(k)
        tables[c] = (sRt, mask)
    solver.close()
    want = ref.compute_sim3(s["kf1"], s["kf2s"], lc.THRESH_MATCHES, lc.THRESH_INLIERS, False, smp, tables=tables)
    rc, got = lc.compute_sim3_call(s["kf1"], s["kf2s"], samples=smp)
    assert rc == _lib.VIEO_OK
    assert got["trace"] == want["trace"] and got["n_visits"] == len(want["trace"])
    assert got["found"] == want["found"] == (kind == "match") and got["cand"] == want["cand"]
    assert got["match12"].tobytes() == want["match12"].tobytes()
    if kind == "match":
        assert got["n_inliers"] == want["n_inliers"]
        exact = _mp_compose(want["S12"], s["kf2s"][want["cand"]])
        own = _compose_error(want["s"], want["R"], want["t"], exact)
        e = _compose_error(got["s"], got["R"], got["t"], exact)
        print("Scw against 50 digits: library %.3g, numpy restatement %.3g" % (e, own))
        assert e <= 8 * own
        mScw = np.concatenate([got["s"] * got["R"], got["t"][:, None]], axis=1).astype(np.float32)
        assert got["Scw"].tobytes() == mScw.tobytes()
    # a trace that is too short: VIEO_E_CAPACITY with the outputs complete
    rc, cut = lc.compute_sim3_call(s["kf1"], s["kf2s"], samples=smp, trace_capacity=2)
    assert rc == _lib.VIEO_E_CAPACITY and cut["trace"] == want["trace"][:2] and cut["n_visits"] == len(want["trace"])
    assert cut["match12"].tobytes() == got["match12"].tobytes() and cut["Scw"].tobytes() == got["Scw"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["match", "fail"])
def test_compute_sim3_end_to_end(kind):
    s = _c_scene(kind)
    smp = _c_samples(kind)
    ok, out = lc.ComputeSim3(s["kf1"], s["kf2s"], s["loop_points_of"], samples=smp)
    rc, raw = lc.compute_sim3_call(s["kf1"], s["kf2s"], samples=smp)
    assert rc == _lib.VIEO_OK and out["cand"] == raw["cand"] and out["trace"] == raw["trace"]
    if kind == "fail":
        assert not ok and out["cand"] == -1 and (out["matched"] == -1).all()
        return
    kf2 = s["kf2s"][raw["cand"]]
    entry = np.where(raw["match12"] >= 0, kf2.mp_id[np.maximum(raw["match12"], 0)], -1).astype(np.int32)
    points, ids = s["loop_points_of"](raw["cand"])
    matched, n = ref.search_by_projection_scw(s["kf1"], raw["Scw"], points, ids, entry, lc.TH_SCW_SEARCH)
    assert out["matched"].tobytes() == matched.tobytes() and out["n_total_matches"] == (matched >= 0).sum()
    assert ok == ((matched >= 0).sum() >= lc.LOOP_MATCHES) and ok


@pytest.mark.gpu
def test_compute_sim3_refuses_bad_arguments():
    s = _c_scene("match")
    smp = _c_samples("match")
    bad = _with_rec(s["kf2s"][1], n_levels=17)
    bad.bow = s["kf2s"][1].bow
    for kw, cands in ((dict(n_rows=0), s["kf2s"]), (dict(n_rows=513), s["kf2s"]), (dict(min_inliers=2), s["kf2s"]),
                      (dict(), [s["kf2s"][0], bad])):
        rc, o = lc.compute_sim3_call(s["kf1"], cands, samples=None if "n_rows" in kw else smp, **kw)
        assert rc == _lib.VIEO_E_INVALID and (o["match12"] == -7).all() and o["n_visits"] == 0, kw
