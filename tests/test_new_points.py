"""LocalMapping::CreateNewMapPoints after the search (reference src/LocalMapping.cc:560-649, :690-806): CPU tests of the
Python reference (tests/new_points_ref.py) on seeded scenes, so that it does not certify itself, and GPU parity of
`vieo_triangulate_new_points` / `vieo_create_new_map_points` (k_tri_new_points) against it.

The GPU tests need the two entries, which the library does not export before this feature: they fail there."""
import os

import numpy as np
import pytest

from tests import new_points_ref as ref
from vieo_slam_amd import tri_search
from vieo_slam_amd.tri_search import (NEWPT_DLT, NEWPT_FAR, NEWPT_LOW_PARALLAX, NEWPT_NO_KEY, NEWPT_SCALE, NEWPT_SKIPPED,
                                      NEWPT_STEREO1, NEWPT_STEREO2, NEWPT_TRI_EMPTY, TriStereo)

BF = 47.9  # make_tri_scene: uright = |x - 47.9 / depth|
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scene_points(seed, n_points=900):
    """the cloud make_tri_scene draws first"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-6, 6, n_points), rng.uniform(-4, 4, n_points), rng.uniform(4, 14, n_points)], 1)


def force_octaves(kf1, kf2, pairs, rig):
    """the scale gate's rows: the key of pKF1 at octave 0, the key of pKF2 at octave 7"""
    for t in pairs:
        i1, i2 = (t[1], t[3]) if rig else t
        kf1.keys["octave"][i1], kf2.keys["octave"][i2] = 0, 7


def truth_rows(kf1, kf2, tr, rig):
    if not rig:
        return np.array(sorted(tr), np.int32).reshape(-1, 2)
    rows = np.full((len(tr), kf1.n_cams + kf2.n_cams), -1, np.int32)
    for r, (c1, i1, c2, i2) in enumerate(sorted(tr)):
        rows[r, c1], rows[r, kf1.n_cams + c2] = i1, i2
    return rows


def shuffled_rows(rows, nc1, n, seed):
    """rows whose pKF2 half comes from another row: wrong partners"""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, len(rows), n), rng.integers(0, len(rows), n)
    out = rows[a].copy()
    out[:, nc1:] = rows[b][:, nc1:]
    return out


def make_case(seed, n_forced=50, **kw):
    """(kf1, st1, kf2s, st2s, truth, forced pairs of neighbour 0): rig key frames get uright = -1 everywhere, as
    Frame.cc:759 leaves them, no depth and no groups"""
    kf1, kf2s, truth = tri_search.make_tri_scene(seed, **kw)
    rig = bool(kw.get("rig"))
    forced = sorted(truth[0])[:n_forced]
    force_octaves(kf1, kf2s[0], forced, rig)
    if rig:
        for k in [kf1] + kf2s:
            k.uright[:] = -1
        mk = lambda k: TriStereo(k, BF, depth=np.full(len(k.keys), -1, np.float32))
    else:
        mk = lambda k: TriStereo(k, BF)
    return kf1, mk(kf1), kf2s, [mk(k) for k in kf2s], truth, forced


def make_rig_stereo_case(seed=8, n_points=400):
    """A rig whose key frames carry stereo data, as a caller has them who fills vuright_ / vdepth_ / the groups for a
    rig (the reference's rig frames leave vuright_ at -1, so its UnprojectStereo branch for rigs only runs then):
    every second scene point of the true pairs gets uright = x - bf / z, depth = z in its own camera, and a group
    whose point is the scene point in the key frame's reference frame.  The stereo baseline is 0.3 m, so that for a
    share of the rows the stereo parallax beats the parallax between the key frames."""
    bf = 0.3 * 458.654
    kf1, kf2s, truth = tri_search.make_tri_scene(seed, rig="radtan", n_points=n_points, n_neighbours=2, pixel_noise=0.2)
    X = scene_points(seed, n_points)
    key_pt = [dict() for _ in range(3)]
    for p, tr in enumerate(truth):
        for (c1, i1, c2, i2), pt in tr.items():
            if pt % 2 == 0:
                key_pt[0][i1], key_pt[1 + p][i2] = pt, pt
    sts = []
    for k, pts in zip([kf1] + kf2s, key_pt):
        T = k.rec[0]["Tcw"].reshape(3, 4)
        k.uright[:] = -1
        depth, grp, p3d = np.full(len(k.keys), -1, np.float32), np.full(len(k.keys), -1, np.int32), []
        for i, pt in sorted(pts.items()):
            Pr = T[:, :3] @ X[pt] + T[:, 3]
            Tcr = k.Tcr[k.key_cam[i]].reshape(3, 4)
            z = Tcr[2, :3] @ Pr + Tcr[2, 3]
            if k.keys["x"][i] - bf / z >= 0:
                k.uright[i], depth[i], grp[i] = k.keys["x"][i] - bf / z, z, len(p3d)
                p3d.append(Pr)
        sts.append(TriStereo(k, bf, baseline=0.3, depth=depth, key_group=grp, group_p3d=np.array(p3d)))
    return kf1, sts[0], kf2s, sts[1:], truth, []


def statuses(res):
    return np.array([r["status"] for r in res], np.int8)


# ------------------------------------------------------------------ the reference itself (CPU)
_ref_runs = {}


def ref_run(oracle, seed):
    """true pairs, 300 rows with shuffled partners per neighbour and the 50 forced-octave rows of one seeded
    undistorted scene, computed once"""
    if seed not in _ref_runs:
        kf1, st1, kf2s, st2s, truth, forced = make_case(seed)
        true = [truth_rows(kf1, k, t, False) for k, t in zip(kf2s, truth)]
        shuf = [shuffled_rows(t, 1, 300, 100 * seed + p) for p, t in enumerate(true)]
        _ref_runs[seed] = dict(case=(kf1, st1, kf2s, st2s), truth=truth, forced=forced, true=true, shuf=shuf,
                               r_true=ref.new_points(oracle, kf1, st1, kf2s, st2s, true),
                               r_shuf=ref.new_points(oracle, kf1, st1, kf2s, st2s, shuf))
    return _ref_runs[seed]


def test_reference_triangulates_true_pairs_of_a_noise_free_scene(oracle):
    """pixel_noise = 0, undistorted: no true pair is lost to the chi2, depth or scale gates (the only reject left is the
    parallax rule for two monocular keys), and an accepted point is within 1e-3 m of the scene point.  The keys are
    float32: rounding of 3e-5 px at 14 m over a 0.18 m baseline is 1e-4 m, the bound leaves a factor of 10."""
    for seed in (0, 1):
        kf1, kf2s, truth = tri_search.make_tri_scene(seed, pixel_noise=0)
        st1, st2s = TriStereo(kf1, BF), [TriStereo(k, BF) for k in kf2s]
        X = scene_points(seed)
        rows = [truth_rows(kf1, k, t, False) for k, t in zip(kf2s, truth)]
        res = ref.new_points(oracle, kf1, st1, kf2s, st2s, rows)
        n_acc = n = 0
        for rr, rw, tr, kf2 in zip(res, rows, truth, kf2s):
            for r, row in zip(rr, rw):
                assert r["status"] in (NEWPT_DLT, NEWPT_STEREO1, NEWPT_STEREO2, NEWPT_LOW_PARALLAX), (row, r)
                n += 1
                if r["status"] >= 0:
                    n_acc += 1
                    assert np.abs(r["x3d"] - X[tr[(int(row[0]), int(row[1]))]]).max() < 1e-3, (row, r)
                    assert np.array_equal(r["x3d_f"], r["x3d"].astype(np.float32))
                else:  # two monocular keys
                    assert kf1.uright[row[0]] < 0 and kf2.uright[row[1]] < 0
        assert n > 500 and n_acc > 0.8 * n


def test_reference_reaches_every_branch(oracle):
    seen, why = set(), set()
    for seed in (0, 1):
        run = ref_run(oracle, seed)
        kf1, st1, kf2s, st2s = run["case"]
        for rr in run["r_true"] + run["r_shuf"]:
            seen |= set(int(r["status"]) for r in rr)
            why |= set(r["why"] for r in rr)
        # wrong partners are mostly caught by the reprojection error or a negative depth
        bad = [r for rr in run["r_shuf"] for r in rr]
        assert sum(r["status"] == NEWPT_TRI_EMPTY for r in bad) > 0.5 * len(bad)
        # the forced octaves (1.2^7 against ratioFactor 1.8) fail the scale gate, or the tighter chi2 of octave 0
        forced = np.array(run["forced"], np.int32).reshape(-1, 2)
        st = statuses(ref.new_points(oracle, kf1, st1, kf2s[:1], st2s[:1], [forced])[0])
        assert (st == NEWPT_SCALE).sum() > 10 and set(st) <= {NEWPT_SCALE, NEWPT_TRI_EMPTY, NEWPT_LOW_PARALLAX}
        seen |= set(int(s) for s in st)
        # th_far_pts = 10 m in a cloud that reaches 14 m
        far = statuses(ref.new_points(oracle, kf1, st1, kf2s[:1], st2s[:1], [run["true"][0]], th_far_pts=10.0)[0])
        near = statuses(run["r_true"][0])
        assert (far == NEWPT_FAR).sum() > 20 and np.array_equal(far[far != NEWPT_FAR], near[far != NEWPT_FAR])
        seen |= set(int(s) for s in far)
        # a row without a key on one side; a neighbour closer than its stereo baseline
        r = ref.new_point_row(ref.KfView(oracle, kf1, st1), ref.KfView(oracle, kf2s[0], st2s[0]), [3, -1])
        assert r["status"] == NEWPT_NO_KEY
        close = TriStereo(kf2s[0], BF, Ow=st1.Ow + np.float32(0.01))
        assert ref.baseline_short(st1, close) and not ref.baseline_short(st1, st2s[0])
        assert set(statuses(ref.new_points(oracle, kf1, st1, kf2s[:1], [close], [run["true"][0]])[0])) == {NEWPT_SKIPPED}
    # (VIEO_NEWPT_ZERO_DIST needs a point in a camera centre, which the positive-depth check before it excludes)
    assert seen >= {NEWPT_DLT, NEWPT_STEREO1, NEWPT_STEREO2, NEWPT_LOW_PARALLAX, NEWPT_TRI_EMPTY, NEWPT_FAR, NEWPT_SCALE}, seen
    assert why >= {"chi2", "depth", "ok"}, why


def test_reference_dlt_known_answer(oracle):
    """null_vector4 of the DLT system of an exact point returns that point"""
    rng = np.random.default_rng(4)
    for n in (2, 3, 8):
        X = np.array([0.7, -1.1, 6.0])
        A = []
        for _ in range(n):
            w = rng.normal(0, 0.05, 3)
            Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
            T = np.concatenate([np.eye(3) + Kx + Kx @ Kx / 2, rng.normal(0, 0.4, (3, 1))], 1)
            Pc = T[:, :3] @ X + T[:, 3]
            A += [Pc[0] / Pc[2] * T[2] - T[0], Pc[1] / Pc[2] * T[2] - T[1]]
        x4 = ref.null_vector4(oracle, np.array(A))
        assert np.abs(x4[:3] / x4[3] - X).max() < 1e-9
        if n <= 4:  # the restatement used beyond the oracle's 8 rows is the oracle's algorithm
            noisy = np.array(A) + rng.normal(0, 1e-3, (2 * n, 4))
            assert np.array_equal(ref.null_vector4_py(noisy), oracle.null_vector4(noisy))


def test_abi_of_the_side_record_and_the_entries():
    import re
    import subprocess
    import sys
    import tempfile
    hdr = open(os.path.join(ROOT, "include", "vieo_hot.h")).read()
    for name in ("vieo_triangulate_new_points", "vieo_create_new_map_points"):
        assert re.search(r"\bint %s\(" % name, hdr), name
    codes = dict(re.findall(r"#define (VIEO_NEWPT_\w+) \(?(-?\d+)\)?", hdr))
    assert len(codes) == 10 and len(set(codes.values())) == 10
    assert int(codes["VIEO_NEWPT_SKIPPED"]) == NEWPT_SKIPPED and int(codes["VIEO_NEWPT_SCALE"]) == NEWPT_SCALE
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "s.c")
        open(src, "w").write('#include <stdio.h>\n#include "vieo_hot.h"\nint main(void) { printf("%zu %zu", '
                             'sizeof(vieo_tri_stereo), sizeof(vieo_tri_keyframe)); return 0; }\n')
        subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), src, "-o", os.path.join(d, "s")])
        a, b = subprocess.check_output([os.path.join(d, "s")]).split()
    assert int(a) == tri_search.TRI_STEREO_DTYPE.itemsize and int(b) == tri_search.TRI_KEYFRAME_DTYPE.itemsize == 232
    assert sys.maxsize > 2 ** 32


# ------------------------------------------------------------------ parity (GPU)
CASES = {
    "seed0": (0, {}), "seed1": (1, {}), "mono": (2, dict(stereo_frac=0.0)), "stereo": (3, dict(stereo_frac=1.0)),
    "radtan": (5, dict(rig="radtan", n_points=700)), "kb8": (6, dict(rig="kb8", n_points=600, n_neighbours=4)),
    "small": (9, dict(n_points=50, n_neighbours=1)), "rig_stereo": (8, dict(rig="radtan")),
}
_gpu_cases = {}


def gpu_case(oracle, name):
    """the case's key frames, the rows of the oracle's search plus the adversarial rows, and the reference's results"""
    if name not in _gpu_cases:
        seed, kw = CASES[name]
        if name == "rig_stereo":
            kf1, st1, kf2s, st2s, truth, forced = make_rig_stereo_case(seed)
        else:
            kf1, st1, kf2s, st2s, truth, forced = make_case(seed, n_forced=50 if name != "small" else 5, **kw)
        rig = bool(kw.get("rig"))
        found = [f[0] for f in oracle.search_for_triangulation(kf1, kf2s)]
        if name == "rig_stereo":  # one key per side: the reference reads idxs.front(), a rig row's first camera
            found = [truth_rows(kf1, k, t, True) for k, t in zip(kf2s, truth)]
        rows = []
        for p, f in enumerate(found):
            parts = [f]
            if len(f) > 1:
                parts.append(shuffled_rows(f, kf1.n_cams, 100 if name != "small" else 10, 7 * seed + p))
            if p == 0 and forced:
                parts.append(truth_rows(kf1, kf2s[0], forced, rig))
            rows.append(np.concatenate(parts).astype(np.int32))
        _gpu_cases[name] = dict(kfs=(kf1, st1, kf2s, st2s), found=found, rows=rows,
                                ref=ref.new_points(oracle, kf1, st1, kf2s, st2s, rows))
    return _gpu_cases[name]


def check_parity(res, got):
    """status equal wherever the reference's margins are outside the bands (1e-6 absolute on the cosine comparisons:
    16 float32 ULP at 1, which covers a contracted float dot or norm; 1e-5 relative on the other gates); at most 2 %
    of the rows inside them; accepted points to 1e-9 relative and x3d_f == float32(x3d).
    Inside the bands on an MI355X: 1 of 1118 rows (seed0), 8 of 1122 (seed1), 3 of 1124 (stereo), 0 in the other cases."""
    n = n_band = n_acc = 0
    for rr, (st, x3d, x3d_f, n_new) in zip(res, got):
        assert len(rr) == len(st)
        assert n_new == int((st >= 0).sum())
        for i, r in enumerate(rr):
            n += 1
            if r["cos_margin"] < ref.COS_BAND or r["rel_margin"] < ref.REL_BAND:
                n_band += 1
                continue
            assert st[i] == r["status"], (i, st[i], r)
            if r["status"] >= 0:
                n_acc += 1
                assert np.abs(x3d[i] - r["x3d"]).max() <= 1e-9 * max(1.0, np.abs(r["x3d"]).max()), (i, x3d[i], r)
        acc = st >= 0
        assert np.array_equal(x3d_f[acc], x3d[acc].astype(np.float32))
        assert not x3d[~acc].any() and not x3d_f[~acc].any()
    print("rows %d, inside the bands %d, accepted %d" % (n, n_band, n_acc))
    assert n_band <= 0.02 * n, (n_band, n)
    return n, n_acc


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_triangulate_new_points_parity(oracle, name):
    c = gpu_case(oracle, name)
    got = tri_search.TriangulateNewPoints(*c["kfs"], c["rows"])
    n, n_acc = check_parity(c["ref"], got)
    assert n_acc > 0.3 * sum(len(f) for f in c["found"])
    if name == "small":
        assert n < 64
    if name in ("radtan", "kb8"):  # rows with more than two keys go through the same DLT
        assert any(((r >= 0).sum(1) > 2).any() for r in c["found"])
    if name == "rig_stereo":  # Twc * v3dpoints_[group] is taken and survives the checks
        assert sum((g[0] == NEWPT_STEREO1).sum() + (g[0] == NEWPT_STEREO2).sum() for g in got) > 10


@pytest.mark.gpu
def test_gpu_far_points_gate(oracle):
    c = gpu_case(oracle, "seed0")
    kf1, st1, kf2s, st2s = c["kfs"]
    rows = [c["found"][0]]
    res = ref.new_points(oracle, kf1, st1, kf2s[:1], st2s[:1], rows, th_far_pts=10.0)
    got = tri_search.TriangulateNewPoints(kf1, st1, kf2s[:1], st2s[:1], rows, th_far_pts=10.0)
    check_parity(res, got)
    assert (got[0][0] == NEWPT_FAR).sum() > 20


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["seed0", "kb8"])
def test_gpu_create_new_map_points_equals_search_then_triangulate(oracle, name):
    from vieo_slam_amd._lib import lib
    kf1, st1, kf2s, st2s = gpu_case(oracle, name)["kfs"]
    rc, pairs, n_pairs, n_matches, status, x3d, x3d_f, n_new = tri_search.create_call(kf1, st1, kf2s, st2s)
    assert rc == 0
    cap, stride, pairs2, n_pairs2, n_matches2, status2, x3d2, x3d_f2, n_new2 = tri_search.new_points_buffers(kf1, kf2s)
    recs = np.concatenate([k.rec for k in kf2s])
    srecs = np.concatenate([s.rec for s in st2s])
    assert lib().vieo_search_for_triangulation(kf1.rec.ctypes.data, recs.ctypes.data, len(kf2s), 0, 1, cap, stride,
                                               pairs2.ctypes.data, n_pairs2.ctypes.data, n_matches2.ctypes.data) == 0
    assert lib().vieo_triangulate_new_points(kf1.rec.ctypes.data, st1.rec.ctypes.data, recs.ctypes.data, srecs.ctypes.data,
                                             len(kf2s), 0.0, cap, stride, pairs2.ctypes.data, n_pairs2.ctypes.data,
                                             status2.ctypes.data, x3d2.ctypes.data, x3d_f2.ctypes.data,
                                             n_new2.ctypes.data) == 0
    for a, b in ((pairs, pairs2), (n_pairs, n_pairs2), (n_matches, n_matches2), (status, status2), (x3d, x3d2),
                 (x3d_f, x3d_f2), (n_new, n_new2)):
        assert a.tobytes() == b.tobytes()
    assert n_new.sum() > 100 and (n_pairs > 0).all()
    out = tri_search.CreateNewMapPoints(kf1, st1, kf2s, st2s)
    assert [len(o[0]) for o in out] == list(n_pairs) and [o[5] for o in out] == list(n_new)


@pytest.mark.gpu
def test_gpu_calls_carry_no_state_from_one_to_the_next(oracle):
    """The driver keeps one call object per thread (its staging blocks, and within a call the device arrays a search
    leaves for the triangulation).  Five calls of different entries, kinds and sizes in one thread, each equal byte for
    byte to the same call made first in a thread of its own, whose call object is new."""
    import threading
    from vieo_slam_amd._lib import lib
    kb8, small, seed0 = (gpu_case(oracle, n) for n in ("kb8", "small", "seed0"))

    def raw(out):  # every output buffer in full
        return [(a.tobytes() if isinstance(a, np.ndarray) else a) for a in out]

    def search_small():
        cap, stride, pairs, n_pairs, n_matches = tri_search.new_points_buffers(small["kfs"][0], small["kfs"][2])[:5]
        recs = np.concatenate([k.rec for k in small["kfs"][2]])
        rc = lib().vieo_search_for_triangulation(small["kfs"][0].rec.ctypes.data, recs.ctypes.data, len(recs), 0, 1, cap, stride,
                                                 pairs.ctypes.data, n_pairs.ctypes.data, n_matches.ctypes.data)
        return rc, pairs, n_pairs, n_matches

    calls = [lambda: tri_search.create_call(*kb8["kfs"]),
             lambda: tri_search.triangulate_call(*small["kfs"], small["rows"]),
             lambda: tri_search.create_call(*seed0["kfs"]),
             search_small,
             lambda: tri_search.triangulate_call(*seed0["kfs"], seed0["rows"])]

    def in_a_new_thread(fns):
        out = []
        t = threading.Thread(target=lambda: out.extend(raw(f()) for f in fns))
        t.start()
        t.join()
        assert len(out) == len(fns)
        return out

    alone = [in_a_new_thread([f])[0] for f in calls]
    together = in_a_new_thread(calls)
    for k, (a, b) in enumerate(zip(alone, together)):
        assert a[0] == 0 and a == b, k
    # the calls did something: rows and new points in both one-call forms, accepted rows in both triangulations
    assert all(np.frombuffer(alone[k][7], np.int32).sum() > 10 for k in (0, 2))
    assert all(np.frombuffer(alone[k][4], np.int32).sum() > 0 for k in (1, 4))
    assert np.frombuffer(alone[3][2], np.int32).sum() > 0


@pytest.mark.gpu
def test_gpu_short_baseline_neighbour_is_skipped(oracle):
    c = gpu_case(oracle, "seed1")
    kf1, st1, kf2s, st2s = c["kfs"]
    close = TriStereo(kf2s[1], BF, Ow=st1.Ow + np.float32(0.01))  # 1.7 cm from pKF1, its stereo baseline is 10 cm
    sts = [st2s[0], close, st2s[2]]
    got = tri_search.TriangulateNewPoints(kf1, st1, kf2s, sts, c["rows"])
    assert set(got[1][0]) == {NEWPT_SKIPPED} and got[1][3] == 0 and not got[1][1].any()
    full = tri_search.TriangulateNewPoints(kf1, st1, kf2s, st2s, c["rows"])
    for p in (0, 2):
        assert all(np.array_equal(a, b) for a, b in zip(got[p][:3], full[p][:3])) and got[p][3] == full[p][3] > 0
    out = tri_search.CreateNewMapPoints(kf1, st1, kf2s, sts)
    assert len(out[1][0]) == 0 and out[1][1] == 0 and out[1][5] == 0  # not searched at all
    alone = tri_search.CreateNewMapPoints(kf1, st1, kf2s, st2s)
    for p in (0, 2):
        assert all(np.array_equal(a, b) for a, b in zip(out[p][:5], alone[p][:5]))


@pytest.mark.gpu
def test_gpu_new_points_edge_cases(oracle):
    from vieo_slam_amd._lib import VIEO_E_CAPACITY, VIEO_E_INVALID, lib
    c = gpu_case(oracle, "seed0")
    kf1, st1, kf2s, st2s = c["kfs"]
    # no neighbours
    assert tri_search.TriangulateNewPoints(kf1, st1, [], [], []) == []
    assert tri_search.create_call(kf1, st1, [], [])[0] == 0
    # a neighbour without rows beside one with 65 (one full wavefront and one lane) and one with 1
    rows = [c["rows"][0][:0], c["rows"][1][:65], c["rows"][2][:1]]
    got = tri_search.TriangulateNewPoints(kf1, st1, kf2s, st2s, rows)
    assert len(got[0][0]) == 0 and got[0][3] == 0
    check_parity([[], c["ref"][1][:65], c["ref"][2][:1]], got)
    # a row without a key on one side
    got = tri_search.TriangulateNewPoints(kf1, st1, kf2s[:1], st2s[:1], [np.array([[3, -1], [-1, 5]], np.int32)])
    assert list(got[0][0]) == [NEWPT_NO_KEY, NEWPT_NO_KEY]
    # capacity: more rows than the buffers hold
    rc = tri_search.triangulate_call(kf1, st1, kf2s, st2s, c["rows"], pair_capacity=5)[0]
    assert rc == VIEO_E_CAPACITY
    assert tri_search.create_call(kf1, st1, kf2s, st2s, pair_capacity=5)[0] == VIEO_E_CAPACITY
    # invalid: a key index out of range, a null record, a rig against undistorted key frames, no depth array
    bad = [np.array([[0, len(kf2s[0].keys)]], np.int32)]
    assert tri_search.triangulate_call(kf1, st1, kf2s[:1], st2s[:1], bad)[0] == VIEO_E_INVALID
    L = lib()
    z = np.zeros(8, np.int64)
    assert L.vieo_triangulate_new_points(kf1.rec.ctypes.data, None, kf2s[0].rec.ctypes.data, st2s[0].rec.ctypes.data, 1,
                                         0.0, 1, 2, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data,
                                         z.ctypes.data, z.ctypes.data) == VIEO_E_INVALID
    assert L.vieo_create_new_map_points(None, st1.rec.ctypes.data, kf2s[0].rec.ctypes.data, st2s[0].rec.ctypes.data, 1,
                                        0, 1, 0.0, 1, 2, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data,
                                        z.ctypes.data, z.ctypes.data, z.ctypes.data) == VIEO_E_INVALID
    r1, rs1, r2s, rs2s = gpu_case(oracle, "radtan")["kfs"]
    assert tri_search.triangulate_call(r1, rs1, kf2s[:1], st2s[:1], [np.zeros((0, 3), np.int32)])[0] == VIEO_E_INVALID
    assert tri_search.create_call(r1, rs1, kf2s[:1], st2s[:1])[0] == VIEO_E_INVALID
    nodepth = TriStereo(kf2s[0], BF)
    nodepth.rec[0]["depth"] = 0
    assert tri_search.triangulate_call(kf1, st1, kf2s[:1], [nodepth], [c["rows"][0]])[0] == VIEO_E_INVALID
