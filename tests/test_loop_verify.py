"""Loop verification, second half, first entry: ORBmatcher::SearchBySim3 for a list of visits in one call
(vieo_search_by_sim3) against the restatement of tests/loop_verify_ref.py.

The CPU tests come first and check the restatement itself, so it does not certify itself: its projection stage against
the oracle's vo_fuse_search on the same flattened inputs (both directions, one camera and the distorted rig), the part
after the searches against a second statement written from the reference's text, on the scenes and on random tables
that reach every branch, and the scenes against their own truth (what is found is a true pair; every planted situation
is there).  The GPU tests ask match12 and nFound bit for bit, and the device stage (best key, best distance per point and
camera) equal to the restatement's."""
import functools

import numpy as np
import pytest

from tests import loop_verify_ref as ref
from vieo_slam_amd import _lib
from vieo_slam_amd import loop_closing as lc


@functools.lru_cache(maxsize=None)
def _scene(kind):
    if kind == "planted":
        return lc.make_loop_pair_scene(11, plant=True)
    if kind == "visits":
        return lc.make_loop_pair_scene(12, n_cands=2)
    return lc.make_loop_pair_scene(13, n_cams=2)


def _entry_match(s, c, every=6):
    """match12 at entry: every sixth true pair is already matched (none of those the scene plants on)"""
    m = np.full(len(s["kf1"].keys), -1, np.int32)
    for i1, i2 in sorted(s["pairs"][c].items())[2::every]:
        m[i1] = i2
    return m


def _perturbed(sim3, k):
    """another Sim3 for the same candidate: the true one turned by 0.4 k degrees, moved by 3 k cm, scaled by 1 + k %"""
    s12, R12, t12 = sim3
    w = np.array([0.004, -0.005, 0.003]) * k
    return np.float32(s12 * (1 + 0.01 * k)), (lc.rodrigues(w) @ R12).astype(np.float32), (t12 + 0.03 * k).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _visits(kind):
    """[(candidate, s12, R12, t12, match12 at entry)] of a scene"""
    s = _scene(kind)
    if kind == "visits":
        return [(0,) + tuple(s["sim3"][0]) + (_entry_match(s, 0),), (0,) + _perturbed(s["sim3"][0], 4) + (_entry_match(s, 0, 9),),
                (1,) + tuple(s["sim3"][1]) + (_entry_match(s, 1),)]
    return [(0,) + tuple(s["sim3"][0]) + (_entry_match(s, 0),)]


@functools.lru_cache(maxsize=None)
def _restated(kind):
    """the restatement on every visit of a scene, once: [(match12, nFound, detail)]"""
    s = _scene(kind)
    return [ref.search_by_sim3(s["kf1"], s["kf2s"][c], s12, R12, t12, m, detail=True) for c, s12, R12, t12, m in _visits(kind)]


# ---------------------------------------------------------------------------------------------------------------------
# CPU
@pytest.mark.parametrize("kind", ["planted", "rig"])
def test_restated_projection_stage_against_the_oracle(oracle, kind):
    s = _scene(kind)
    kf1, kf2 = s["kf1"], s["kf2s"][0]
    (_, _, d), = _restated(kind)
    for src, dst, (R, t), am, got in ((kf1, kf2, d["transforms"][0], d["am"][0], d["fwd"]),
                                      (kf2, kf1, d["transforms"][1], d["am"][1], d["bwd"])):
        bi, bd = ref.oracle_project_stage(oracle, src, dst, R, t, lc.TH_SIM3, am)
        assert (bi >= 0).sum() > 60
        assert np.array_equal(bi, got[0]) and np.array_equal(bd, got[1])


def test_restated_transforms_are_the_sim3_and_its_inverse():
    s = _scene("visits")
    kf1, kf2 = s["kf1"], s["kf2s"][0]
    s12, R12, t12 = (np.asarray(a, np.float64) for a in s["sim3"][0])
    (Ra, ta), (Rb, tb) = ref.sim3_transforms(kf1, kf2, *s["sim3"][0])
    R1, t1, R2, t2 = (np.asarray(a, np.float64) for a in (kf1.Rcw, kf1.tcw, kf2.Rcw, kf2.tcw))
    assert np.abs(Rb - s12 * R12 @ R2).max() < 1e-6 and np.abs(tb - (s12 * R12 @ t2 + t12)).max() < 1e-5
    assert np.abs(Ra - R12.T @ R1 / s12).max() < 1e-6 and np.abs(ta - R12.T @ (t1 - t12) / s12).max() < 1e-5
    # a map point of the current key frame lands on its physical twin in the candidate's frame
    i1, i2 = sorted(s["pairs"][0].items())[0]
    X2 = R2 @ kf2.points[i2]["Xw"] + t2
    assert np.abs(Ra.astype(np.float64) @ kf1.points[i1]["Xw"] + ta - X2).max() < 1e-4


@pytest.mark.parametrize("kind", ["planted", "visits", "rig"])
def test_restated_walk_against_the_brute_force_statement(kind):
    s = _scene(kind)
    for (c, _, _, _, m), (out, n_found, d) in zip(_visits(kind), _restated(kind)):
        out2, n2 = ref.search_by_sim3_brute(s["kf1"], s["kf2s"][c], d["fwd"], d["bwd"], m)
        assert np.array_equal(out, out2) and n_found == n2 and n_found > 40


def test_restated_walk_on_random_tables():
    """random (best key, distance) tables on the rig scene: keys without a map point win or lose a camera, distances
    around TH_HIGH, agreement through either key of a map point"""
    s = _scene("rig")
    kf1, kf2 = s["kf1"], s["kf2s"][0]
    rng = np.random.default_rng(5)
    taken = 0
    for _ in range(20):
        tabs = []
        for src, dst in ((kf1, kf2), (kf2, kf1)):
            n = len(src.keys)
            bi = rng.integers(-1, len(dst.keys), (n, dst.n_cams)).astype(np.int32)
            bd = np.where(bi >= 0, rng.integers(60, 140, bi.shape), ref.INT_MAX).astype(np.int32)
            twin = {int(m) % 1000: k for k, m in enumerate(dst.mp_id) if m >= 0}
            for i in np.flatnonzero(src.mp_id >= 0)[::2]:  # half the points see their physical twin in one camera
                if int(src.mp_id[i]) % 1000 in twin:
                    bi[i, rng.integers(0, dst.n_cams)] = twin[int(src.mp_id[i]) % 1000]
            bd = np.where(bi >= 0, np.where(bd == ref.INT_MAX, 90, bd), ref.INT_MAX).astype(np.int32)
            tabs.append((bi, bd))
        m = np.full(len(kf1.keys), -1, np.int32)
        vn0, vn1 = ref.only_one_match(kf1, kf2, *tabs[0]), ref.only_one_match(kf2, kf1, *tabs[1])
        out, n_found = ref.agreement(vn0, vn1, m)
        out2, n2 = ref.search_by_sim3_brute(kf1, kf2, tabs[0], tabs[1], m)
        assert np.array_equal(out, out2) and n_found == n2
        taken += n_found
    assert taken > 100


def test_the_scene_holds_what_it_plants():
    s = _scene("planted")
    kf1, kf2 = s["kf1"], s["kf2s"][0]
    (c, _, _, _, m), = _visits("planted")
    (out, n_found, d), = _restated("planted")
    pairs, P = s["pairs"][0], s["planted"]
    # what is found is a true pair, and most true pairs that were open are found
    new = np.flatnonzero((out != m))
    assert all(pairs[int(i1)] == int(out[i1]) for i1 in new) and len(new) == n_found and n_found > 60
    # pairs matched at entry are skipped on both sides and stay
    for i1 in np.flatnonzero(m >= 0):
        assert d["fwd"][0][i1, 0] == -1 and d["bwd"][0][m[i1], 0] == -1 and out[i1] == m[i1]
    # a forward hit without backward agreement
    a1 = P["no_backward"]
    assert m[a1] < 0 and d["vn"][0][a1] == [pairs[a1]] and a1 not in d["vn"][1][pairs[a1]] and out[a1] == -1
    # the best key holds no map point while a worse one in the window does: nothing is taken
    b1, free, b2 = P["best_without_point"]
    assert m[b1] < 0 and d["fwd"][0][b1, 0] == free and kf2.mp_id[free] < 0 and d["vn"][0][b1] == [] and out[b1] == -1
    assert d["bwd"][0][b2, 0] == b1  # (the worse key would have agreed)
    # keys 0.1 % inside / outside the window
    (in1, in2), (out1, out2) = P["edge_in"], P["edge_out"]
    assert d["fwd"][0][in1, 0] == in2 and d["fwd"][0][out1, 0] != out2


def test_the_rig_scene_has_a_map_point_in_both_cameras():
    s = _scene("rig")
    kf1, kf2 = s["kf1"], s["kf2s"][0]
    (out, n_found, d), = _restated("rig")
    both = [m for m in set(kf2.mp_id[kf2.mp_id >= 0].tolist()) if len(set(kf2.cam_of_key[kf2.mp_id == m].tolist())) == 2]
    assert len(both) > 30 and kf1.use_distort and (np.diff(kf1.cam_of_key) < 0).any()
    # some current key is matched through a list of two keys, and some is matched in a camera that is not its own
    assert any(len(v) == 2 for v in d["vn"][0]) and n_found > 40
    assert any(out[i1] >= 0 and kf2.cam_of_key[out[i1]] != kf1.cam_of_key[i1] for i1 in range(len(out)))


# ---------------------------------------------------------------------------------------------------------------------
# GPU
def _device(kind, visits=None):
    s = _scene(kind)
    return lc.SearchBySim3(s["kf1"], s["kf2s"], _visits(kind) if visits is None else visits)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["planted", "visits", "rig"])
def test_search_by_sim3_equals_the_restatement(kind):
    s = _scene(kind)
    got = _device(kind)
    for v, ((c, _, _, _, m), (out, n_found, d), (g_out, g_found)) in enumerate(zip(_visits(kind), _restated(kind), got)):
        for direction, want in ((0, d["fwd"]), (1, d["bwd"])):
            bi, bd = lc.search_by_sim3_tap(s["kf1"], s["kf2s"][c], v, direction)
            assert np.array_equal(bi, want[0]) and np.array_equal(bd, want[1]), (v, direction)
        assert g_found == n_found and g_out.tobytes() == out.tobytes()


@pytest.mark.gpu
def test_search_by_sim3_visits_one_by_one_and_again():
    """two visits of candidate 0 with different Sim3 and one of candidate 1: one call, the single calls and a second call
    return the same bytes; the two visits of candidate 0 differ"""
    batch = _device("visits")
    again = _device("visits")
    for v, visit in enumerate(_visits("visits")):
        (m1, f1), = _device("visits", [visit])
        assert m1.tobytes() == batch[v][0].tobytes() == again[v][0].tobytes() and f1 == batch[v][1] == again[v][1]
    assert batch[0][0].tobytes() != batch[1][0].tobytes()


@pytest.mark.gpu
def test_search_by_sim3_invalid_arguments_touch_nothing():
    s = _scene("visits")
    kf1, kf2s = s["kf1"], s["kf2s"]
    c, s12, R12, t12, m = _visits("visits")[0]
    _device("visits")  # a valid call: its tap must survive the refused ones
    tap = lc.search_by_sim3_tap(kf1, kf2s[0], 0, 0)

    def refused(kf1_, kf2s_, visits):
        before = [np.array(v[4], np.int32) for v in visits]
        rc, out = lc.search_by_sim3_call(kf1_, kf2s_, visits)
        assert rc == _lib.VIEO_E_INVALID
        assert all(o[0].tobytes() == b.tobytes() and o[1] == 0 for o, b in zip(out, before))
        now = lc.search_by_sim3_tap(kf1, kf2s[0], 0, 0)
        assert now[0].tobytes() == tap[0].tobytes() and now[1].tobytes() == tap[1].tobytes()

    bad = m.copy()
    bad[5] = len(kf2s[0].keys)
    refused(kf1, kf2s, [(c, s12, R12, t12, m), (c, s12, R12, t12, bad)])  # a match12 entry outside the candidate's keys
    refused(kf1, kf2s, [(2, s12, R12, t12, m)])                           # a candidate outside the table
    refused(kf1, kf2s, [(c, np.float32(0), R12, t12, m)])                 # no scale

    def broken(field, value, index=None):
        k = lc.LoopKeyFrame(kf2s[1].bow, kf2s[1].points, np.eye(4), kf2s[1].cam_of_key)
        k.rec[:] = kf2s[1].rec
        if index is None:
            k.rec[field] = value
        else:
            k.rec[field][0][index] = value
        return k
    refused(kf1, [kf2s[0], broken("n_levels", 17)], [(c, s12, R12, t12, m)])
    refused(kf1, [kf2s[0], broken("n_cams", 2)], [(c, s12, R12, t12, m)])
    refused(kf1, [kf2s[0], broken("points", 0)], [(c, s12, R12, t12, m)])
    refused(kf1, [kf2s[0], broken("bounds", 100.0, (0, 1))], [(c, s12, R12, t12, m)])
    cam = kf2s[1].cams.copy()
    cam[0]["model"] = 7
    k = broken("cams", cam.ctypes.data)
    refused(kf1, [kf2s[0], k], [(c, s12, R12, t12, m)])
    octave = lc.LoopKeyFrame(lc.BowKeys(kf2s[1].keys.copy(), kf2s[1].desc, [], kf2s[1].mp_id), kf2s[1].points, np.eye(4))
    octave.keys["octave"][3] = 8
    refused(kf1, [kf2s[0], octave], [(c, s12, R12, t12, m)])
    of_cam = lc.LoopKeyFrame(kf2s[1].bow, kf2s[1].points, np.eye(4), np.full(len(kf2s[1].keys), 1, np.int32))
    refused(kf1, [kf2s[0], of_cam], [(c, s12, R12, t12, m)])
