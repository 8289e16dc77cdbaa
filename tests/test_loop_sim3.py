"""Loop verification, first half: ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*) and Sim3Solver for batches of loop
candidates (vieo_search_by_bow_kf, vieo_sim3_*) against the restatement of tests/loop_ref.py.

The CPU tests come first and check the restatement itself (against the truth of the generated scenes, against a
brute-force statement, and against the device's arithmetic compiled for the host), so it does not certify itself.  The
reference computes Horn's closed form in CV_32F with cv::eigen; the library and the restatement compute it in FP64, so
parity is asked between those two (1e-9, the bound of the FP64 EPnP in test_relocalization.py), on every row whose two
largest eigenvalues of N lie at least 1e-3 apart (relative): below that the eigenvector itself is ill-conditioned.

Figures of the CPU run: restated Horn on 400 noise-free triples 2.2e-14; host build of the device's Horn against the
restatement 2.9e-13 on 1278 of 1280 rows (2 excused by the gap), CheckInliers bit for bit; restated RANSAC on seeds
100 ... 131 (60 correspondences, 20 % outliers, 1 cm): worst error against the truth E_t = 0.1901 m, E_R = 0.02172 rad,
E_s = 0.00433, first success at rows 0 ... 5; the hard scene (60 % outliers) succeeds at row 12, in the third
iterate(5).  Device: Horn against the restatement 1.3e-13 on 280 rows (none excused), 2 of 17 680 mask entries next to a
threshold, the RANSAC's worst error equal to the restatement's."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import loop_ref as ref
from vieo_slam_amd import _lib
from vieo_slam_amd import loop_closing as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = list(range(100, 132))
ROWS = 40
PARAMS = lc.LOOP_SIM3_PARAMS
GAP = 1e-3


def _scene_samples(seed, rows=ROWS):
    s = lc.make_sim3_scene(seed, fix_scale=bool(seed & 1))
    return s, lc.draw_samples(np.random.default_rng([seed, 1]), len(s["X1"]), rows)


@functools.lru_cache(maxsize=None)
def _hard_scene():
    """60 % gross outliers: 24 true matches of 60 against mRansacMinInliers = 20"""
    s = lc.make_sim3_scene(900, 60, 0.6, 0.01)
    return s, lc.draw_samples(np.random.default_rng([900, 1]), 60, 128)


def _decompose(T12):
    """(R, t, s) of a 4 x 4 [s R | t]"""
    A = np.asarray(T12, np.float64)[:3, :3]
    s = float(np.cbrt(np.linalg.det(A)))
    return A / s, np.asarray(T12, np.float64)[:3, 3], s


def _truth_error(T12, s):
    return ref.sim3_error(*_decompose(T12), s["R12"], s["t12"], s["s12"])


@functools.lru_cache(maxsize=None)
def _ransac_restated():
    """the restated RANSAC on every seed, once: [(result of find(), error against the truth)]"""
    out = []
    for seed in SEEDS:
        s, samples = _scene_samples(seed, 128)
        solver = ref.Sim3SolverRef(s, samples, PARAMS)
        r = solver.find()
        out.append((r, _truth_error(r.T12, s) if r.found else (np.inf,) * 3, solver.min_inliers, solver.max_its))
    return out


def _worst_restated_error():
    errs = [e for _, e, _, _ in _ransac_restated()]
    return tuple(max(e[k] for e in errs) for k in range(3))


# ---------------------------------------------------------------------------------------------------------------------
# CPU
def _spread_triple(rng):
    """3 points at 4-12 m whose triangle has sides of at least 1 m and no angle below 20 degrees"""
    while True:
        P = rng.uniform([-4, -3, 4], [4, 3, 12], (3, 3))
        e = [P[1] - P[0], P[2] - P[1], P[0] - P[2]]
        ln = [np.linalg.norm(v) for v in e]
        cs = [-(e[i] @ e[(i + 1) % 3]) / (ln[i] * ln[(i + 1) % 3]) for i in range(3)]
        if min(ln) >= 1.0 and max(cs) <= np.cos(np.radians(20)):
            return P


def test_restated_horn_recovers_the_generating_sim3():
    rng = np.random.default_rng(11)
    worst = 0.0
    for k in range(400):
        fix = bool(k & 1)
        R0, t0 = lc.rodrigues(rng.standard_normal(3) * 0.5), rng.standard_normal(3)
        s0 = 1.0 if fix else float(rng.uniform(0.5, 2.0))
        P2 = _spread_triple(rng)
        P1 = s0 * P2 @ R0.T + t0
        R, t, s, gap = ref.horn_sim3(P1, P2, fix)
        assert gap > GAP
        worst = max(worst, np.abs(R - R0).max(), np.abs(t - t0).max(), abs(s - s0))
        if fix:
            assert s == 1.0
    print("worst error of the restated Horn on noise-free triples: %.3g" % worst)
    assert worst <= 1e-9


def test_restated_ransac_finds_a_sim3_on_every_seed():
    runs = _ransac_restated()
    for seed, (r, err, min_inliers, max_its) in zip(SEEDS, runs):
        assert (min_inliers, max_its) == (20, 123), seed
        assert r.found and not r.no_more and r.n_inliers > 20, seed
    E = _worst_restated_error()
    print("restated RANSAC: worst error %.4f m / %.5f rad / %.5f of scale, first success at rows %d ... %d"
          % (E + (min(r.row for r, _, _, _ in runs), max(r.row for r, _, _, _ in runs))))
    assert E[0] < 0.5 and E[1] < 0.05 and E[2] < 0.02  # 1 cm of noise on 3 points a few metres apart, seen from 4-12 m
    # the hard scene: the first success lies past row 5, so one iterate(5) does not reach it
    s, samples = _hard_scene()
    solver = ref.Sim3SolverRef(s, samples, PARAMS)
    calls, r = 0, None
    while r is None or not (r.found or r.no_more):
        r, calls = solver.iterate(5), calls + 1
    print("hard scene: %d true matches, success at row %d after %d calls of iterate(5)" % (s["truth"].sum(), r.row, calls))
    assert r.found and r.row > 5 and calls > 1
    assert max(_truth_error(r.T12, s)[:2]) < 0.5


def test_ransac_parameters_truncate_like_the_reference():
    assert ref.ransac_parameters(60, 0.99, 20, 300) == (20, 123)   # epsilon 1/3: ceil(122.02)
    assert ref.ransac_parameters(25, 0.99, 20, 300) == (20, 7)     # epsilon 0.8: ceil(6.42)
    assert ref.ransac_parameters(300, 0.99, 20, 300) == (20, 300)  # ceil(15541) capped
    assert ref.ransac_parameters(20, 0.99, 20, 300) == (20, 1)     # N == mRansacMinInliers
    assert ref.ransac_parameters(3, 0.99, 3, 300) == (3, 1)
    assert ref.ransac_parameters(19, 0.99, 20, 300) == (20, 1)     # N < mRansacMinInliers: no solver
    assert lc.max_error(np.float32(1.2) ** (2 * np.arange(4))).tolist() == [9, 13, 19, 27]  # 9.21, 13.26, 19.10, 27.50


def test_draw_samples_is_swap_with_back():
    class Fixed:  # always position 0 of the list of available indices
        def integers(self, lo, hi):
            return 0
    assert lc.draw_samples(Fixed(), 10, 2).tolist() == [[0, 9, 8], [0, 9, 8]]
    rows = lc.draw_samples(np.random.default_rng(3), 9, 200)
    assert rows.min() == 0 and rows.max() == 8 and all(len(set(r)) == 3 for r in rows.tolist())


def test_sim3_correspondences_restates_the_constructor():
    """a rig's map point with two keys in the candidate gives two correspondences with one index1; NULL and bad points
    on either side give none; the thresholds are integers"""
    sigma2 = (np.float32(1.2) ** np.arange(8)).astype(np.float32) ** 2
    Pw = {7: [0.5, 0.2, 5.0], 8: [1.0, -0.3, 6.0], 9: [-1.0, 0.1, 7.0], 17: [0.5, 0.2, 5.1], 18: [1.0, -0.3, 6.1]}
    T2 = np.eye(4)
    T2[:3, 3] = [0.1, 0.0, -0.2]
    c = lc.sim3_correspondences(mp_id1=[7, -1, 8, 9], matched12=[17, 18, -1, 18], index_in_kf2={17: [4], 18: [2, -1, 6]},
                                Pw=Pw, Tcw1=np.eye(4), Tcw2=T2, octave1=[0, 1, 2, 3], octave2=[0, 0, 1, 1, 2, 2, 3],
                                level_sigma2_1=sigma2, level_sigma2_2=sigma2, cam_of_key1=[0, 0, 1, 1],
                                cam_of_key2=[0, 0, 0, 0, 1, 1, 1], fix_scale=True)
    assert c["index1"].tolist() == [0, 3, 3] and c["n1"] == 4 and c["fix_scale"]
    assert c["max_err1"].tolist() == [9, 27, 27] and c["max_err2"].tolist() == [19, 13, 27]
    assert c["cam1"].tolist() == [0, 1, 1] and c["cam2"].tolist() == [1, 0, 1]
    assert np.allclose(c["X1"], [Pw[7], Pw[9], Pw[9]]) and np.allclose(c["X2"][0], [0.6, 0.2, 4.9])
    assert c["X1"].dtype == np.float32 and c["max_err1"].dtype == np.int32


def test_restated_search_by_bow_kf_against_brute_force():
    kf1, cands = lc.make_bow_kf_scene(1)
    assert len(cands) == 3 and len(kf1.keys) == 300 and len(kf1.feat_vec) == 40 and all(len(k.keys) == 300 for k in cands)
    total = dict(skipped=0, no_point=0, ratio=0, replaced=0, kept=0, rotation=0)
    for p, kf2 in enumerate(cands):
        for check in (True, False):
            m, n, ev = ref.search_by_bow_kf(kf1, kf2, 0.75, check)
            m2, n2, _ = ref.search_by_bow_kf_brute(kf1, kf2, 0.75, check)
            assert np.array_equal(m, m2) and n == n2
            if p == len(cands) - 1:  # no shared node
                assert n == 0 and (m == -1).all()
                continue
            assert n > 40
            held = kf2.mp_id[m[m >= 0]]
            assert (held >= 0).all() and (kf1.mp_id[m >= 0] >= 0).all()  # both ends of a match hold a map point
            for k in total:
                total[k] += ev[k]
    # every order-dependent rule of the walk fires: a candidate key already matched or without a map point is skipped,
    # the ratio test rejects, the (map point, 0) table replaces and keeps, the rotation histogram removes
    assert all(v > 0 for v in total.values()), total


def _tables_from_restatement(s, samples):
    sRt, mask = np.zeros((len(samples), 13)), np.zeros((len(samples), len(s["X1"])), bool)
    for r, idx in enumerate(samples):
        R, t, sc, _ = ref.horn_sim3(s["X1"][idx].astype(np.float64), s["X2"][idx].astype(np.float64), s["fix_scale"])
        sRt[r, :9], sRt[r, 9:12], sRt[r, 12] = R.reshape(-1), t, sc
        mask[r] = ref.check_inliers(R, t, sc, s)
    return sRt, mask


def _same(a, b, what):
    assert a.found == b.found and a.no_more == b.no_more and a.n_inliers == b.n_inliers and a.row == b.row, what
    assert np.array_equal(a.inliers, b.inliers), what
    if a.found:
        assert a.T12.tobytes() == b.T12.tobytes(), what


def test_iterate_over_tables_equals_the_sequential_iterate():
    """all rows ahead, iterate as look-ups -- against Sim3Solver::iterate restated statement by statement, call by call.
    The hard scene has rows of equal count before its first success (the later row becomes the best) and, with
    mRansacMinInliers = 23, a row of exactly 23 inliers, which becomes the best and is not returned."""
    hard, hard_samples = _hard_scene()
    cases = [_scene_samples(seed) + (PARAMS,) for seed in SEEDS[:4]]
    cases += [(hard, hard_samples, PARAMS), (hard, hard_samples, dict(PARAMS, min_inliers=23))]
    ties = exact = 0
    for s, samples, params in cases:
        sRt, mask = _tables_from_restatement(s, samples)
        solver = ref.Sim3SolverRef(s, samples, params)
        replay = ref.Sim3SolverRef(s, samples, params, tables=(sRt, mask))
        count = mask.sum(axis=1)
        for call in range(6):
            before = solver.iterations
            a, b = solver.iterate(5), replay.iterate(5)
            _same(a, b, call)
            assert (solver.iterations, solver.best_inliers, solver.best_row) == (replay.iterations, replay.best_inliers, replay.best_row)
            for x, y in zip(solver.estimate(), replay.estimate()):
                assert np.array_equal(x, y)
            for r in range(before, solver.iterations):
                ties += r > 0 and count[r] == count[:r].max() and solver.best_row >= r
                exact += count[r] == solver.min_inliers and count[r] >= count[:r + 1].max() and not (a.found and a.row == r)
    assert ties > 0 and exact > 0, (ties, exact)


@functools.lru_cache(maxsize=None)
def _emul():
    """tests/emul/sim3_emul.cc: the lane functions of the kernel (csrc/sim3_solver_device.h) compiled for the host"""
    out = os.path.join(ROOT, "tests", "emul", "libsim3_emul.so")
    csrc = os.path.join(ROOT, "vieo_slam_amd", "csrc")
    deps = [os.path.join(ROOT, "tests", "emul", "sim3_emul.cc"), os.path.join(csrc, "sim3_solver_device.h"),
            os.path.join(csrc, "cam_project.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", out, deps[0], "-lm"])
    L = ctypes.CDLL(out)
    L.emul_sim3_check.restype = ctypes.c_int
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)

    def horn(P1, P2, fix_scale):
        a, b, o = np.ascontiguousarray(P1, np.float32), np.ascontiguousarray(P2, np.float32), np.zeros(13)
        L.emul_sim3_horn(vp(a), vp(b), int(fix_scale), vp(o))
        return o[:9].reshape(3, 3).copy(), o[9:12].copy(), float(o[12])

    def check(R, t, sc, s):
        n = len(s["X1"])
        o = np.concatenate([np.asarray(R, np.float64).reshape(-1), np.asarray(t, np.float64), [float(sc)]])
        words = np.zeros((1, (n + 63) // 64), np.uint64)
        cnt = L.emul_sim3_check(vp(s["X1"]), vp(s["X2"]), vp(s["max_err1"]), vp(s["max_err2"]), vp(s["cam1"]), vp(s["cam2"]), n,
                                vp(s["cams1"]), vp(s["cams2"]), vp(o), vp(words))
        return cnt, lc._unpack_masks(words, n)[0]

    return horn, check


def _pose_difference(got, want):
    """max |difference| of R, t, s between two (R, t, s)"""
    return max(np.abs(got[0] - want[0]).max(), np.abs(got[1] - want[1]).max(), abs(got[2] - want[2]))


def test_device_arithmetic_on_the_host_against_the_restatement():
    """the kernel's lane functions as plain C++: Horn's closed form with the Jacobi eigen-solver against LAPACK on 1280
    hypotheses (rows whose top eigenvalue gap is below 1e-3 are excused and counted), CheckInliers bit for bit --
    also on the two rigs --, the whole RANSAC on the first seeds"""
    horn, check = _emul()
    worst, excused, total = 0.0, 0, 0
    for seed in SEEDS:
        s, samples = _scene_samples(seed)
        for idx in samples:
            R, t, sc = horn(s["X1"][idx], s["X2"][idx], s["fix_scale"])
            want = ref.horn_sim3(s["X1"][idx].astype(np.float64), s["X2"][idx].astype(np.float64), s["fix_scale"])
            total += 1
            assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-9 and np.linalg.det(R) > 0
            assert sc == 1.0 or not s["fix_scale"]
            n, mask = check(R, t, sc, s)
            assert np.array_equal(mask, ref.check_inliers(R, t, sc, s)) and n == mask.sum()
            if want[3] < GAP:
                excused += 1
                continue
            worst = max(worst, _pose_difference((R, t, sc), want))
    print("host build of the device Horn vs restatement: %.3g on %d of %d rows (%d excused by the gap)"
          % (worst, total - excused, total, excused))
    assert total == 1280 and worst <= 1e-9 and excused <= 0.01 * total
    for n_cams in (2, 4):
        s = lc.make_sim3_scene(500 + n_cams, 80, 0.2, 0.01, n_cams=n_cams)
        for idx in lc.draw_samples(np.random.default_rng([n_cams, 1]), 80, ROWS):
            R, t, sc = horn(s["X1"][idx], s["X2"][idx], s["fix_scale"])
            n, mask = check(R, t, sc, s)
            assert np.array_equal(mask, ref.check_inliers(R, t, sc, s)) and n == mask.sum()
    E = _worst_restated_error()
    for seed in SEEDS[:8]:
        s, samples = _scene_samples(seed, 128)
        r = ref.Sim3SolverRef(s, samples, PARAMS, horn=lambda a, b, f: horn(a, b, f)).find()
        assert r.found and all(e <= 3 * w for e, w in zip(_truth_error(r.T12, s), E))


# ---------------------------------------------------------------------------------------------------------------------
# GPU
def _check_table(s, samples, sRt, count, mask, what):
    """the properties of a table of hypotheses: R orthonormal with det > 0, R / t / s = the restatement's on the row's
    3 pairs unless the eigenvalue gap excuses the row, the mask = the restated CheckInliers at the device's own pose
    except next to a threshold, the count = the mask's popcount.
    returns (rows, rows excused, worst difference, entries, entries excused)"""
    me1, me2 = s["max_err1"].astype(np.float64), s["max_err2"].astype(np.float64)
    rows_excused, worst, entries, excused = 0, 0.0, 0, 0
    for r in range(len(sRt)):
        R, t, sc = sRt[r, :9].reshape(3, 3), sRt[r, 9:12], sRt[r, 12]
        assert count[r] == mask[r].sum(), (what, r)
        assert np.isfinite(sRt[r]).all() and np.abs(R.T @ R - np.eye(3)).max() <= 1e-9 and np.linalg.det(R) > 0, (what, r)
        idx = samples[r]
        want = ref.horn_sim3(s["X1"][idx].astype(np.float64), s["X2"][idx].astype(np.float64), s["fix_scale"])
        if want[3] < GAP:
            rows_excused += 1
        else:
            d = _pose_difference((R, t, sc), want)
            assert d <= 1e-9, (what, r, d)
            worst = max(worst, d)
        if s["fix_scale"]:
            assert sc == 1.0, (what, r)
        err1, err2 = ref.sim3_errors(R, t, sc, s)
        with np.errstate(all="ignore"):
            near = (np.abs(err1.astype(np.float64) / me1 - 1.0) < 1e-4) | (np.abs(err2.astype(np.float64) / me2 - 1.0) < 1e-4)
            want_mask = (err1 < me1.astype(np.float32)) & (err2 < me2.astype(np.float32))
        differ = mask[r] != want_mask
        assert not (differ & ~near).any(), (what, r, np.flatnonzero(differ & ~near))
        entries += len(err1)
        excused += int(near.sum())
    return len(sRt), rows_excused, worst, entries, excused


@pytest.mark.gpu
def test_search_by_bow_kf_parity():
    kf1, cands = lc.make_bow_kf_scene(1)
    assert len(cands) == 3 and len(kf1.keys) == 300 and len(kf1.feat_vec) == 40
    assert not set(dict(kf1.feat_vec)) & set(dict(cands[2].feat_vec))  # a key frame with no shared node
    replaced = no_point = 0
    for check in (True, False):
        got = lc.SearchByBoWKF(kf1, cands, 0.75, check)  # all 3 candidates in one call
        for kf2, (match12, n) in zip(cands, got):
            m, n_ref, ev = ref.search_by_bow_kf(kf1, kf2, 0.75, check)
            assert np.array_equal(match12, m) and n == n_ref
            replaced, no_point = replaced + ev["replaced"], no_point + ev["no_point"]
        assert got[2][1] == 0 and (got[2][0] == -1).all()
    assert replaced > 0 and no_point > 0  # a replaced entry of the (map point, 0) table; a candidate key without a map point


@pytest.mark.gpu
def test_sim3_rows_table():
    sizes = [3, 19, 60, 64, 65, 130, 60, 60]
    scenes = []
    for seed, n in zip(SEEDS[:8], sizes):
        s = lc.make_sim3_scene(seed, n, fix_scale=bool(seed & 1))
        scenes.append((s, lc.draw_samples(np.random.default_rng([seed, 1]), n, ROWS)))
    assert {s["fix_scale"] for s, _ in scenes[2:]} == {False, True}
    solver = lc.Sim3Solver([s for s, _ in scenes], [smp for _, smp in scenes], params=PARAMS)
    three = lc.Sim3Solver([scenes[0][0]], [scenes[0][1]], params=dict(PARAMS, min_inliers=3))
    rows = rows_x = entries = excused = 0
    worst = 0.0
    for c, (s, smp) in enumerate(scenes):
        info = solver.info(c)
        samples, sRt, count, mask = solver.rows(c)
        assert (info["n"], info["n1"], info["n_rows"], info["mask_words"]) == (sizes[c], s["n1"], ROWS, (sizes[c] + 63) // 64)
        if sizes[c] < 20:  # below mRansacMinInliers: no rows, bNoMore at once
            assert (info["min_inliers"], info["max_its"]) == (20, 1)
            assert not sRt.any() and not count.any() and not mask.any()
            r = solver.iterate(c, 5)
            assert r.no_more and not r.found and solver.info(c)["iterations"] == 0 and solver.estimate(c) is None
            continue
        assert (info["min_inliers"], info["max_its"]) == ref.ransac_parameters(sizes[c], **PARAMS)
        assert np.array_equal(samples, smp)
        a, b, w, e, x = _check_table(s, smp, sRt, count, mask, "seed %d" % SEEDS[c])
        rows, rows_x, worst, entries, excused = rows + a, rows_x + b, max(worst, w), entries + e, excused + x
    # N == mRansacMinInliers = 3: one iteration
    s, smp = scenes[0]
    info = three.info(0)
    assert (info["min_inliers"], info["max_its"], info["mask_words"]) == (3, 1, 1)
    samples, sRt, count, mask = three.rows(0)
    a, b, w, e, x = _check_table(s, smp, sRt, count, mask, "n = 3")
    rows, rows_x, worst, entries, excused = rows + a, rows_x + b, max(worst, w), entries + e, excused + x
    r = three.iterate(0, 5)
    assert three.info(0)["iterations"] == 1 and r.no_more == (not r.found)
    print("rows: %d, %d excused by the gap (%.4f), worst R / t / s difference %.3g; mask entries: %d, %d next to a "
          "threshold (%.5f)" % (rows, rows_x, rows_x / rows, worst, entries, excused, excused / entries))
    assert rows == 7 * ROWS and rows_x <= 0.01 * rows and excused <= 0.01 * entries


@pytest.mark.gpu
@pytest.mark.parametrize("n_cams", [2, 4])
def test_sim3_rig_cameras(n_cams):
    """the 2-camera Radtan and the 4-camera KB8 rig: per-correspondence camera indices on both sides, correspondences
    that share their index1"""
    s = lc.make_sim3_scene(500 + n_cams, 80, 0.2, 0.01, n_cams=n_cams)
    assert len(s["cams1"]) == n_cams and set(s["cam1"].tolist()) == set(range(n_cams)) and (s["cam1"] != s["cam2"]).any()
    assert len(set(s["index1"].tolist())) < len(s["index1"]) == 80
    smp = lc.draw_samples(np.random.default_rng([n_cams, 1]), 80, ROWS)
    solver = lc.Sim3Solver([s], [smp], params=PARAMS)
    samples, sRt, count, mask = solver.rows(0)
    rows, rows_x, worst, entries, excused = _check_table(s, smp, sRt, count, mask, "rig %d" % n_cams)
    assert excused <= 0.01 * entries and (count > 20).any()
    replay = ref.Sim3SolverRef(s, smp, PARAMS, tables=(sRt, mask))
    r, want = solver.iterate(0, 5), replay.iterate(5)
    _same(r, want, n_cams)
    assert r.found and r.inliers.sum() <= r.n_inliers  # (several correspondences of one key set one flag)
    flags = np.zeros(s["n1"], bool)
    flags[s["index1"][mask[r.row]]] = True
    assert np.array_equal(r.inliers, flags)


def _same_state(solver, c, replay):
    info = solver.info(c)
    assert (info["iterations"], info["best_inliers"], info["best_row"]) == (replay.iterations, replay.best_inliers, replay.best_row)
    got, want = solver.estimate(c), replay.estimate()
    assert (got is None) == (want is None)
    if got is not None:
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(got, want))


@pytest.mark.gpu
def test_sim3_iterate_is_the_replay_of_its_tables():
    scenes = [_scene_samples(seed, 128) for seed in SEEDS] + [_hard_scene()]
    solver = lc.Sim3Solver([s for s, _ in scenes], [smp for _, smp in scenes], params=PARAMS)
    for c, (s, smp) in enumerate(scenes):
        _, sRt, _, mask = solver.rows(c)
        replay = ref.Sim3SolverRef(s, smp, PARAMS, tables=(sRt, mask))
        _same_state(solver, c, replay)
        calls = 0
        while True:
            r, want = solver.iterate(c, 5), replay.iterate(5)
            _same(r, want, (c, calls))
            _same_state(solver, c, replay)
            calls += 1
            if r.found or r.no_more:
                break
        assert r.found and (c < len(SEEDS) or calls > 1)  # the hard scene takes more than one iterate(5)
        _same(solver.find(c), replay.find(), (c, "find"))  # on from where iterate stopped, up to mRansacMaxIts
        _same_state(solver, c, replay)
    # a table shorter than the rows a call needs
    s, smp = _hard_scene()
    short = lc.Sim3Solver([s], [smp[:8]], params=PARAMS)
    rc, r = short.iterate_call(0, 5)
    assert rc == _lib.VIEO_OK and not r.found and not r.no_more and short.info(0)["iterations"] == 5
    rc, r = short.iterate_call(0, 5)
    assert rc == _lib.VIEO_E_CAPACITY and not r.found and short.info(0)["iterations"] == 8


@pytest.mark.gpu
def test_sim3_outcome():
    E = _worst_restated_error()
    scenes = [_scene_samples(seed, 128) for seed in SEEDS]
    runs = []
    for _ in range(2):
        solver = lc.Sim3Solver([s for s, _ in scenes], [smp for _, smp in scenes], params=PARAMS)
        runs.append([(solver.find(c), solver.rows(c)) for c in range(len(scenes))])
    worst = [0.0, 0.0, 0.0]
    for c, (s, _) in enumerate(scenes):
        r = runs[0][c][0]
        assert r.found and not r.no_more and r.n_inliers > 20, SEEDS[c]
        worst = [max(w, e) for w, e in zip(worst, _truth_error(r.T12, s))]
        _same(r, runs[1][c][0], SEEDS[c])
        for a, b in zip(runs[0][c][1], runs[1][c][1]):
            assert a.tobytes() == b.tobytes(), SEEDS[c]  # two runs on the same inputs: the same bytes
    print("device RANSAC: worst error %.4f m / %.5f rad / %.5f of scale (restatement %.4f / %.5f / %.5f)" % (tuple(worst) + E))
    assert all(w <= 3 * e for w, e in zip(worst, E))


@pytest.mark.gpu
def test_sim3_library_draws_from_a_seed():
    s = lc.make_sim3_scene(100)
    a, b, c = (lc.Sim3Solver([s], n_rows=128, seed=seed, params=PARAMS) for seed in (5, 5, 6))
    rows = a.rows(0)[0]
    assert rows.min() >= 0 and rows.max() < 60 and all(len(set(r)) == 3 for r in rows.tolist())
    for x, y in zip(a.rows(0), b.rows(0)):
        assert x.tobytes() == y.tobytes()
    assert not np.array_equal(rows, c.rows(0)[0])
    assert a.find(0).found


@pytest.mark.gpu
def test_sim3_invalid_arguments_touch_nothing():
    s = lc.make_sim3_scene(100)
    L = _lib.lib()
    par = lc._params_record(PARAMS)
    good = lc.draw_samples(np.random.default_rng(0), 60, ROWS)

    def create(scene=s, samples=None, n_rows=ROWS, params=par, n_cands=1, null=None, **override):
        cand = lc._Candidate(dict(scene, **override))
        rec = cand.record()
        h = ctypes.c_void_p(12345)
        rc = L.vieo_sim3_create(ctypes.byref(h), None if null == "cands" else rec.ctypes.data, n_cands,
                                None if null == "params" else params.ctypes.data,
                                samples.ctypes.data if samples is not None else None, n_rows, 0)
        return rc, h.value

    bad = (_lib.VIEO_E_INVALID, None)
    assert L.vieo_sim3_create(None, None, 1, par.ctypes.data, None, ROWS, 0) == _lib.VIEO_E_INVALID
    assert create(null="cands") == bad and create(null="params") == bad
    assert create(n_cands=0) == bad and create(n_cands=-1) == bad
    assert create(n_rows=0) == bad and create(n_rows=513) == bad
    index1 = s["index1"].copy()
    index1[5] = s["n1"]
    assert create(index1=index1) == bad
    index1[5] = -1
    assert create(index1=index1) == bad
    cam = s["cam1"].copy()
    cam[9] = 1  # the table has one camera
    assert create(cam1=cam) == bad and create(cam2=cam) == bad
    smp = good.copy()
    smp[7, 2] = 60  # out of range
    assert create(samples=smp) == bad
    smp[7, 2] = smp[7, 0]  # drawn twice
    assert create(samples=smp) == bad
    assert create(params=lc._params_record(dict(PARAMS, min_inliers=2))) == bad  # below the minimal set
    rec = lc._Candidate(s).record()
    rec["X2"] = 0
    h = ctypes.c_void_p(12345)
    assert L.vieo_sim3_create(ctypes.byref(h), rec.ctypes.data, 1, par.ctypes.data, None, ROWS, 0) == _lib.VIEO_E_INVALID
    assert h.value is None
    # iterate / get_estimate / tap with a bad candidate index or a null output: the outputs keep their sentinel
    solver = lc.Sim3Solver([s], [good], params=PARAMS)
    T12, inl = np.full(16, -7, np.float32), np.full(s["n1"], 7, np.uint8)
    found, n_inl, no_more, row = (ctypes.c_int32(-7) for _ in range(4))
    for cand, fp in ((1, ctypes.byref(found)), (-1, ctypes.byref(found)), (0, None)):
        rc = L.vieo_sim3_iterate(solver._h, cand, 5, fp, T12.ctypes.data, inl.ctypes.data, ctypes.byref(n_inl),
                                 ctypes.byref(no_more), ctypes.byref(row))
        assert rc == _lib.VIEO_E_INVALID
    assert (T12 == -7).all() and (inl == 7).all() and [v.value for v in (found, n_inl, no_more, row)] == [-7] * 4
    assert solver.info(0)["iterations"] == 0 and solver.estimate(0) is None
    # SearchByBoW(KF, KF): a feature index out of range, a key angle of 360, no candidate
    kf1, cands = lc.make_bow_kf_scene(1)
    recs = np.concatenate([k.rec for k in cands])
    match, n_matches = np.full((3, 300), -7, np.int32), np.full(3, -7, np.int32)

    def search(a, b, n):
        return L.vieo_search_by_bow_kf(a.ctypes.data if a is not None else None, b.ctypes.data, n, 0.75, 1, match.ctypes.data,
                                       n_matches.ctypes.data)

    assert search(None, recs, 3) == _lib.VIEO_E_INVALID and search(kf1.rec, recs, 0) == _lib.VIEO_E_INVALID
    feat = cands[1].node_feat.copy()
    feat[3] = 300
    broken = recs.copy()
    broken[1]["node_feat"] = feat.ctypes.data
    assert search(kf1.rec, broken, 3) == _lib.VIEO_E_INVALID
    keys = kf1.keys.copy()
    keys["angle"][10] = 360.0
    turned = kf1.rec.copy()
    turned["keys"] = keys.ctypes.data
    assert search(turned, recs, 3) == _lib.VIEO_E_INVALID
    assert (match == -7).all() and (n_matches == -7).all()
    assert search(kf1.rec, recs, 3) == _lib.VIEO_OK and (n_matches[:2] > 40).all() and n_matches[2] == 0
