"""Relocalisation of a lost frame: ORBmatcher::SearchByBoW(KeyFrame*, Frame&) and PnPsolver for batches of candidates
(vieo_search_by_bow, vieo_pnp_*) against the restatement of tests/reloc_ref.py.

The CPU tests come first and check the restatement itself (against the truth of the generated scenes, against a
brute-force statement, and against the device's arithmetic compiled for the host), so it does not certify itself.
A 4-point hypothesis of the reference is not defined beyond round-off (MtM has a 4-dimensional null space), so the GPU
tests ask for parity where the reference is defined -- EPnP for n >= 6, CheckInliers, the selection logic, SearchByBoW --
and for properties where it is not.

Figures of the host build of the device arithmetic (tests/emul/pnp_emul.cc), CPU: EPnP for n = 6 ... 60 with 0.5 px of
noise agrees with the LAPACK restatement to 4.4e-14 m / 5.5e-15 rad on the 60 inlier sets of the refine case; of the 400
noise-free 4-point sets it recovers 0.4475, the restatement 0.4425.  Restated RANSAC on seeds 100 ... 131: worst pose error
E_t = 0.0235 m, E_R = 0.00288 rad, latest first success at row 15 of 35."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import reloc_ref as ref
from vieo_slam_amd import _lib
from vieo_slam_amd import relocalization as rl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = list(range(100, 132))
ROWS = 40
PARAMS = rl.RELOC_PNP_PARAMS


def _scene_samples(seed):
    s = rl.make_pnp_scene(seed)
    return s, rl.draw_samples(np.random.default_rng([seed, 1]), len(s["Xw"]), ROWS)


def _ref_solver(s, samples, solver=ref.epnp):
    return ref.PnPSolverRef(s["Xw"], s["uv"], s["sigma2"], s["key_index"], s["n_frame_keys"], s["K"], samples, PARAMS,
                            solver=solver)


@functools.lru_cache(maxsize=None)
def _ransac_restated():
    """the restated RANSAC on every seed, once: [(result of the first iterate(5), pose error against the truth)]"""
    out = []
    for seed in SEEDS:
        s, samples = _scene_samples(seed)
        solver = _ref_solver(s, samples)
        r = solver.iterate(5)
        err = ref.pose_error(r.Tcw[:3, :3], r.Tcw[:3, 3], s["R"], s["t"]) if r.found else (np.inf, np.inf)
        out.append((r, err, solver.min_inliers, solver.max_its))
    return out


def _worst_restated_error():
    errs = [e for _, e, _, _ in _ransac_restated()]
    return max(e[0] for e in errs), max(e[1] for e in errs)


@functools.lru_cache(maxsize=None)
def _four_point_sets():
    """400 noise-free all-inlier 4-point sets (seed 7) and the share the restatement recovers to 1e-3 m / 1e-3 rad"""
    rng = np.random.default_rng(7)
    sets = [rl.make_pnp_scene(0, 4, 0.0, 0.0, rng=rng) for _ in range(400)]
    ok = 0
    for s in sets:
        R, t = ref.epnp(s["Xw"].astype(np.float64), s["uv"].astype(np.float64), s["K"])
        ok += max(ref.pose_error(R, t, s["R"], s["t"])) < 1e-3
    return sets, ok / len(sets)


def _refine_case():
    """one noisy all-inlier scene of 60 correspondences and 60 inlier sets of 6 ... 60 of them"""
    s = rl.make_pnp_scene(77, 60, 0.0, 0.5)
    rng = np.random.default_rng(78)
    masks = np.zeros((60, 60), bool)
    for i in range(60):
        masks[i, rng.choice(60, 6 + (i * 54) // 59, replace=False)] = True
    return s, masks


# ---------------------------------------------------------------------------------------------------------------------
# CPU
def test_restated_epnp_recovers_the_true_pose():
    rng = np.random.default_rng(11)
    worst = 0.0
    for n in (6, 8, 20, 60):
        for _ in range(50):
            s = rl.make_pnp_scene(0, n, 0.0, 0.0, rng=rng)
            R, t = ref.epnp(s["Xw"].astype(np.float64), s["uv"].astype(np.float64), s["K"])
            worst = max(worst, *ref.pose_error(R, t, s["R"], s["t"]))
    print("worst error of the restated EPnP on noise-free sets: %.3g" % worst)
    assert worst <= 1e-4


def test_restated_ransac_returns_a_pose_on_every_seed():
    runs = _ransac_restated()
    for seed, (r, err, min_inliers, max_its) in zip(SEEDS, runs):
        assert (min_inliers, max_its) == (30, 35), seed
        assert r.found and not r.no_more, seed
    E_t, E_R = _worst_restated_error()
    print("restated RANSAC: worst pose error %.4f m / %.5f rad, latest first success at row %d"
          % (E_t, E_R, max(r.row for r, _, _, _ in runs)))
    assert E_t < 0.1 and E_R < 0.02  # 0.5 px of noise at 1.5-12 m: centimetres and milliradians


def test_ransac_parameters_truncate_like_the_reference():
    assert ref.ransac_parameters(60, 0.99, 10, 300, 4, 0.5) == (30, 35)
    assert ref.ransac_parameters(20, 0.99, 10, 300, 4, 0.5) == (10, 35)
    assert ref.ransac_parameters(15, 0.99, 10, 300, 4, 0.5) == (10, 14)  # int(7.5) = 7 < 10; epsilon -> 10 / 15: ceil(13.1)
    assert ref.ransac_parameters(4, 0.99, 4, 300, 4, 0.5) == (4, 1)      # mRansacMinInliers == N


def test_draw_samples_is_swap_with_back():
    class Fixed:  # always position 0 of the list of available indices
        def integers(self, lo, hi):
            return 0
    rows = rl.draw_samples(Fixed(), 10, 2)
    assert rows.tolist() == [[0, 9, 8, 7], [0, 9, 8, 7]]
    rows = rl.draw_samples(np.random.default_rng(3), 9, 200)
    assert rows.min() == 0 and rows.max() == 8 and all(len(set(r)) == 4 for r in rows.tolist())


def test_restated_search_by_bow_against_brute_force():
    frame, kfs = rl.make_bow_scene(1)
    assert len(kfs) == 3 and len(frame.keys) == 300 and all(len(k.keys) == 300 for k in kfs)
    total = dict(skipped=0, ratio=0, replaced=0, kept=0, rotation=0)
    for kf in kfs:
        for check in (True, False):
            m, n, ev = ref.search_by_bow(kf, frame, 0.75, check)
            m2, n2, _ = ref.search_by_bow_brute(kf, frame, 0.75, check)
            assert np.array_equal(m, m2) and n == n2
            assert n == int((m >= 0).sum()) > 40
            held = kf.mp_id[m[m >= 0]]
            assert (held >= 0).all() and len(set(held.tolist())) == len(held)  # a map point is matched once
            for k in total:
                total[k] += ev[k]
    # every order-dependent rule of the walk fires: a frame key already matched is skipped, the ratio test rejects,
    # the (map point, image) table replaces, the rotation histogram removes
    assert total["skipped"] > 0 and total["ratio"] > 0 and total["replaced"] > 0 and total["rotation"] > 0, total


def test_principal_direction_sign_moves_only_the_noisy_pose():
    """cv::SVD leaves the sign of the control points' principal directions to its internals.  The library and the
    restatement fix it (largest component positive), so on that one point the parity reference is aligned with the code
    under test; this shows what the convention decides: nothing without noise, the noise level with it."""
    rng = np.random.default_rng(21)
    clean = noisy = 0.0
    for _ in range(20):
        for noise in (0.0, 0.5):
            s = rl.make_pnp_scene(0, 20, 0.0, noise, rng=rng)
            pw, us = s["Xw"].astype(np.float64), s["uv"].astype(np.float64)
            R0, t0 = ref.epnp(pw, us, s["K"])
            for flip in ((-1, 1, 1), (1, -1, 1), (1, 1, -1), (-1, -1, -1)):
                d = max(ref.pose_error(*ref.epnp(pw, us, s["K"], direction_signs=flip), R0, t0))
                if noise:
                    noisy = max(noisy, d)
                else:
                    clean = max(clean, d)
    print("flipping a principal direction moves the pose by %.3g without noise, %.3g with 0.5 px" % (clean, noisy))
    assert clean <= 1e-4 and noisy > 1e-4


def _tables_from_restatement(s, samples):
    """what the two device passes produce, built with ref.epnp / ref.check_inliers: a row per sample, a record per row
    that raises the best-so-far inlier set"""
    solver = _ref_solver(s, samples)
    Xw, uv = s["Xw"].astype(np.float64), s["uv"].astype(np.float64)
    Rt, count, mask = np.zeros((len(samples), 12)), np.zeros(len(samples), np.int32), np.zeros((len(samples), len(Xw)), bool)
    for r, idx in enumerate(samples):
        R, t = ref.epnp(Xw[idx], uv[idx], solver.K)
        Rt[r, :9], Rt[r, 9:] = R.reshape(-1), t
        mask[r] = ref.check_inliers(R, t, solver.Xw, solver.uv, solver.max_err, solver.K)
        count[r] = mask[r].sum()
    rec_row, rec_Rt, rec_count, rec_mask, best = [], [], [], [], 0
    for r in range(len(samples)):
        if count[r] >= solver.min_inliers and count[r] > best:
            best = count[r]
            idx = np.flatnonzero(mask[r])
            R, t = ref.epnp(Xw[idx], uv[idx], solver.K)
            m = ref.check_inliers(R, t, solver.Xw, solver.uv, solver.max_err, solver.K)
            rec_row.append(r), rec_Rt.append(np.concatenate([R.reshape(-1), t])), rec_count.append(m.sum()), rec_mask.append(m)
    replay = ref.IterateReplay((Rt, count, mask), (np.array(rec_row), rec_Rt, np.array(rec_count), rec_mask),
                               solver.min_inliers, solver.max_its, s["key_index"], s["n_frame_keys"])
    return solver, replay, count, np.array(rec_row), np.array(rec_count)


def test_iterate_over_tables_equals_the_sequential_iterate():
    """all rows ahead, Refine once per record, iterate as look-ups -- against PnPsolver::iterate restated
    statement by statement (PnPSolverRef), call by call.  The last scene has so few true matches that Refine fails on a
    record (its count is not above mRansacMinInliers) and later rows below the best re-enter Refine on the same set."""
    cases = [_scene_samples(seed) for seed in SEEDS[:6]]
    hard = rl.make_pnp_scene(900, 60, 0.5, 0.1)  # 30 true matches of 60 = mRansacMinInliers: Refine cannot exceed it
    cases.append((hard, rl.draw_samples(np.random.default_rng([900, 1]), 60, 400)))
    refine_failed = reentered = 0
    for s, samples in cases:
        solver, replay, count, rec_row, rec_count = _tables_from_restatement(s, samples)
        for call in range(70 if s is hard else 4):  # also past bNoMore: five more rows a call
            _same(solver.iterate(5), replay.iterate(5), call)
        assert solver.iterations == replay.iterations
        failed = rec_row[rec_count <= solver.min_inliers]
        refine_failed += len(failed)
        for r in failed:  # a later visited row that qualifies without raising the best
            later = [q for q in range(r + 1, solver.iterations) if count[q] >= solver.min_inliers and q not in rec_row]
            reentered += len(later)
    assert refine_failed > 0 and reentered > 0, (refine_failed, reentered)


@functools.lru_cache(maxsize=None)
def _chain_case(kind):
    """a relocalisation scene, its sample tables (48 rows per candidate, indices below the candidate's BoW matches)"""
    seed = {"widen": 1, "direct": 2, "none": 3, "narrow": 4}[kind]
    frame, cands, truth = rl.make_reloc_scene(seed, kind)
    n = [int((ref.search_by_bow(c.bow, frame.bow, 0.75, True)[0] >= 0).sum()) for c in cands]
    samples = [rl.draw_samples(np.random.default_rng([seed, i]), max(k, 4), 48) for i, k in enumerate(n)]
    return frame, cands, truth, samples


def _took_widening_search(trace):
    return any(v["n_additional"][0] >= 0 for v in trace)


def test_restated_chain(oracle):
    # Widen: 45 true + 8 false BoW matches are too few for 50 inliers; the th = 10 search finds the other 120 points
    frame, cands, truth, samples = _chain_case("widen")
    out = ref.relocalize(frame, cands, samples, ref.RefPnPBatch, oracle, PARAMS)
    assert out["found"] and out["cand"] == 0 and out["n_good"] >= 150 and _took_widening_search(out["trace"])
    assert max(ref.pose_error(out["Tcw"][:3, :3], out["Tcw"][:3, 3], truth["R"], truth["t"])) < 0.02
    stage0 = {v["cand"]: v for v in out["trace"] if v["call"] == 0}
    assert stage0[0]["n_inliers"] == 53 and stage0[1]["n_inliers"] < 15 and stage0[1]["no_more"] == 1
    assert stage0[2]["n_inliers"] == 20 and stage0[2]["no_more"] == 0
    assert not any(v["cand"] == 1 and v["call"] > 0 for v in out["trace"])  # discarded: never iterated
    held = out["mp_ref"][out["mp_ref"] >= 0]
    assert len(held) >= 150 and len(set(held.tolist())) == len(held) and not out["outlier"][out["mp_ref"] >= 0].any()
    # the candidate with 20 matches anywhere: alone, it ends in bNoMore without a pose
    alone = ref.relocalize(frame, cands[2:], samples[2:], ref.RefPnPBatch, oracle, PARAMS)
    assert not alone["found"] and [(v["call"], v["no_more"], v["found"]) for v in alone["trace"]] == [(0, 0, 0), (1, 1, 0)]
    # Direct: 120 true + 15 false matches, success after the first optimisation
    frame, cands, truth, samples = _chain_case("direct")
    out = ref.relocalize(frame, cands, samples, ref.RefPnPBatch, oracle, PARAMS)
    assert out["found"] and out["n_good"] >= 110 and not _took_widening_search(out["trace"])
    assert out["trace"][-1]["n_good"][1:] == [-1, -1]
    # None: every candidate is discarded, by SearchByBoW or by bNoMore
    frame, cands, truth, samples = _chain_case("none")
    out = ref.relocalize(frame, cands, samples, ref.RefPnPBatch, oracle, PARAMS)
    assert not out["found"] and (out["mp_ref"] == -1).all() and not out["outlier"].any()
    last = {v["cand"]: v for v in out["trace"]}
    assert len(last) == 3 and all(v["no_more"] for v in last.values()) and not any(v["found"] for v in out["trace"])
    # the fourth scene: the second optimisation lands between 30 and 50, the th = 3 search runs
    frame, cands, truth, samples = _chain_case("narrow")
    out = ref.relocalize(frame, cands, samples, ref.RefPnPBatch, oracle, PARAMS)
    assert any(30 < v["n_good"][1] < 50 and v["n_additional"][1] >= 0 for v in out["trace"])


@functools.lru_cache(maxsize=None)
def _emul():
    """tests/emul/pnp_emul.cc: the lane functions of the two kernels (csrc/pnp_device.h) compiled for the host"""
    out = os.path.join(ROOT, "tests", "emul", "libpnp_emul.so")
    deps = [os.path.join(ROOT, "tests", "emul", "pnp_emul.cc"), os.path.join(ROOT, "vieo_slam_amd", "csrc", "pnp_device.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", out, deps[0], "-lm"])
    L = ctypes.CDLL(out)
    L.emul_pnp_check.restype = ctypes.c_int

    def epnp(pw, us, K):
        Xw, uv = np.ascontiguousarray(pw, np.float32), np.ascontiguousarray(us, np.float32)
        Kf, idx, Rt = np.array(K, np.float32), np.arange(len(Xw), dtype=np.int32), np.zeros(12)
        L.emul_pnp_epnp(*(ctypes.c_void_p(a.ctypes.data) for a in (Xw, uv)), len(Xw), ctypes.c_void_p(Kf.ctypes.data),
                        ctypes.c_void_p(idx.ctypes.data), len(idx), ctypes.c_void_p(Rt.ctypes.data))
        return Rt[:9].reshape(3, 3).copy(), Rt[9:].copy()

    def check(R, t, Xw, uv, max_err, K):
        Xw, uv, me = (np.ascontiguousarray(a, np.float32) for a in (Xw, uv, max_err))
        Kf, Rt = np.array(K, np.float32), np.concatenate([np.asarray(R, np.float64).reshape(-1), np.asarray(t, np.float64)])
        words = np.zeros((1, (len(Xw) + 63) // 64), np.uint64)
        n = L.emul_pnp_check(*(ctypes.c_void_p(a.ctypes.data) for a in (Xw, uv, me)), len(Xw), ctypes.c_void_p(Kf.ctypes.data),
                             ctypes.c_void_p(Rt.ctypes.data), ctypes.c_void_p(words.ctypes.data))
        return n, rl._unpack_masks(words, len(Xw))[0]

    return epnp, check


def test_device_arithmetic_on_the_host_against_the_restatement():
    """the kernels' lane functions as plain C++: Jacobi eigen-solver + Householder least squares + polar factor against
    LAPACK for n >= 6 (where EPnP is defined), CheckInliers bit for bit, the whole RANSAC on the first seeds"""
    epnp, check = _emul()
    s, masks = _refine_case()
    worst_t = worst_R = 0.0
    for m in masks:
        idx = np.flatnonzero(m)
        R, t = epnp(s["Xw"][idx], s["uv"][idx], s["K"])
        R0, t0 = ref.epnp(s["Xw"][idx].astype(np.float64), s["uv"][idx].astype(np.float64), s["K"])
        dt, dR = ref.pose_error(R, t, R0, t0)
        worst_t, worst_R = max(worst_t, dt), max(worst_R, dR)
        assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-9 and np.linalg.det(R) > 0
        max_err = ref.max_error(s["sigma2"], PARAMS["th2"])
        n, mask = check(R, t, s["Xw"], s["uv"], max_err, s["K"])
        assert np.array_equal(mask, ref.check_inliers(R, t, s["Xw"], s["uv"], max_err, s["K"])) and n == mask.sum()
    print("host build of the device EPnP vs restatement, n = 6 ... 60: %.3g m, %.3g rad" % (worst_t, worst_R))
    assert worst_t <= 1e-9 and worst_R <= 1e-9
    E_t, E_R = _worst_restated_error()
    for seed in SEEDS[:8]:
        sc, samples = _scene_samples(seed)
        r = _ref_solver(sc, samples, solver=epnp).iterate(5)
        assert r.found
        dt, dR = ref.pose_error(r.Tcw[:3, :3], r.Tcw[:3, 3], sc["R"], sc["t"])
        assert dt <= 3 * E_t and dR <= 3 * E_R


# ---------------------------------------------------------------------------------------------------------------------
# GPU
def _check_tables(s, Rt, count, mask, what):
    """the properties of a pose table: R orthogonal with det > 0, the mask = the restated CheckInliers at the device's
    own pose except next to the threshold, the count = the mask's popcount.  returns (finite rows, entries, excused)"""
    max_err = ref.max_error(s["sigma2"], PARAMS["th2"])
    finite = entries = excused = 0
    for r in range(len(Rt)):
        R, t = Rt[r, :9].reshape(3, 3), Rt[r, 9:]
        assert count[r] == mask[r].sum(), (what, r)
        if not np.isfinite(Rt[r]).all():
            assert count[r] == 0, (what, r)
            continue
        finite += 1
        assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-9 and np.linalg.det(R) > 0, (what, r)
        with np.errstate(all="ignore"):
            e2 = ref.reprojection_error2(R, t, s["Xw"], s["uv"], s["K"])
            near = np.abs(e2.astype(np.float64) / max_err.astype(np.float64) - 1.0) < 1e-4
        differ = mask[r] != (e2 < max_err)
        assert not (differ & ~near).any(), (what, r, np.flatnonzero(differ & ~near))
        entries += len(e2)
        excused += int(near.sum())
    return finite, entries, excused


@pytest.mark.gpu
def test_search_by_bow_parity():
    frame, kfs = rl.make_bow_scene(1)
    for check in (True, False):
        got = rl.SearchByBoW(kfs, frame, 0.75, check)  # all 3 candidates in one call
        for kf, (match, n) in zip(kfs, got):
            m, n_ref, _ = ref.search_by_bow(kf, frame, 0.75, check)
            assert np.array_equal(match, m) and n == n_ref


@pytest.mark.gpu
def test_pnp_hypotheses_table():
    seeds = SEEDS[:8]
    scenes = [_scene_samples(seed) for seed in seeds]
    solver = rl.PnPSolver([s for s, _ in scenes], [smp for _, smp in scenes], params=PARAMS)
    finite = entries = excused = 0
    for c, (s, smp) in enumerate(scenes):
        info = solver.info(c)
        assert (info["min_inliers"], info["max_its"], info["n_rows"], info["mask_words"]) == (30, 35, ROWS, 1)
        samples, Rt, count, mask = solver.rows(c)
        assert np.array_equal(samples, smp)
        f, e, x = _check_tables(s, Rt, count, mask, "seed %d" % seeds[c])
        finite, entries, excused = finite + f, entries + e, excused + x
    print("pass A: %d of %d rows finite, %d of %d entries next to the threshold" % (finite, 8 * ROWS, excused, entries))
    assert finite > 0.9 * 8 * ROWS and excused <= 0.01 * entries


@pytest.mark.gpu
def test_pnp_minimal_solve_quality():
    sets, share_ref = _four_point_sets()
    minimal = dict(PARAMS, min_inliers=4)  # N = 4 = mRansacMinInliers: one row, the 4 points themselves
    solver = rl.PnPSolver(sets, [np.array([[0, 1, 2, 3]], np.int32)] * len(sets), params=minimal)
    ok = 0
    for c, s in enumerate(sets):
        _, Rt, _, _ = solver.rows(c)
        if np.isfinite(Rt[0]).all():
            ok += max(ref.pose_error(Rt[0, :9].reshape(3, 3), Rt[0, 9:], s["R"], s["t"])) < 1e-3
    share = ok / len(sets)
    print("4-point sets recovered: device %.4f, restatement %.4f" % (share, share_ref))
    assert share >= 0.8 * share_ref


@pytest.mark.gpu
def test_pnp_refine_parity():
    s, masks = _refine_case()
    Rt, count, out = rl.PnPSolver.refine_masks(s, masks, PARAMS)
    worst_t = worst_R = 0.0
    for i, m in enumerate(masks):
        idx = np.flatnonzero(m)
        R0, t0 = ref.epnp(s["Xw"][idx].astype(np.float64), s["uv"][idx].astype(np.float64), s["K"])
        dt, dR = ref.pose_error(Rt[i, :9].reshape(3, 3), Rt[i, 9:], R0, t0)
        worst_t, worst_R = max(worst_t, dt), max(worst_R, dR)
    print("pass B vs restated EPnP, n_inl = 6 ... 60: %.3g m, %.3g rad" % (worst_t, worst_R))
    assert worst_t <= 1e-9 and worst_R <= 1e-9
    finite, entries, excused = _check_tables(s, Rt, count, out, "refine")
    assert finite == len(masks) and excused <= 0.01 * entries


def _replay(solver, c, s):
    info = solver.info(c)
    _, Rt, count, mask = solver.rows(c)
    return ref.IterateReplay((Rt, count, mask), solver.records(c), info["min_inliers"], info["max_its"], s["key_index"],
                             s["n_frame_keys"])


def _same(a, b, what):
    assert a.found == b.found and a.no_more == b.no_more and a.n_inliers == b.n_inliers and a.row == b.row, what
    if a.found:
        assert a.Tcw.tobytes() == b.Tcw.tobytes() and np.array_equal(a.inliers, b.inliers), what


@pytest.mark.gpu
def test_pnp_iterate_is_the_replay_of_its_tables():
    scenes = [_scene_samples(seed) for seed in SEEDS]
    # one more candidate: 20 matches whose pixels are random
    rng = np.random.default_rng(5)
    junk = rl.make_pnp_scene(99, 20, 1.0, 0.5)
    scenes.append((junk, rl.draw_samples(rng, 20, ROWS)))
    solver = rl.PnPSolver([s for s, _ in scenes], [smp for _, smp in scenes], params=PARAMS)
    for c, (s, _) in enumerate(scenes[:-1]):
        replay = _replay(solver, c, s)
        for call in range(3):
            _same(solver.iterate(c, 5), replay.iterate(5), (SEEDS[c], call))
        assert solver.info(c)["iterations"] == replay.iterations
    c = len(scenes) - 1
    info = solver.info(c)
    assert (info["min_inliers"], info["max_its"]) == (10, 35)
    r = solver.iterate(c, 5)
    _same(r, _replay(solver, c, junk).iterate(5), "junk")
    assert r.no_more and not r.found and r.Tcw is None and solver.info(c)["iterations"] == 35


@pytest.mark.gpu
def test_pnp_outcome():
    E_t, E_R = _worst_restated_error()
    scenes = [_scene_samples(seed) for seed in SEEDS]
    runs = []
    for _ in range(2):
        solver = rl.PnPSolver([s for s, _ in scenes], [smp for _, smp in scenes], params=PARAMS)
        runs.append([(solver.iterate(c, 5), solver.rows(c), solver.records(c)) for c in range(len(scenes))])
    worst_t = worst_R = 0.0
    for c, (s, _) in enumerate(scenes):
        r = runs[0][c][0]
        assert r.found and not r.no_more and r.n_inliers > 30, SEEDS[c]
        dt, dR = ref.pose_error(r.Tcw[:3, :3], r.Tcw[:3, 3], s["R"], s["t"])
        worst_t, worst_R = max(worst_t, dt), max(worst_R, dR)
        _same(r, runs[1][c][0], SEEDS[c])
        for a, b in zip(runs[0][c][1] + runs[0][c][2], runs[1][c][1] + runs[1][c][2]):
            assert a.tobytes() == b.tobytes(), SEEDS[c]  # two runs on the same inputs: the same bytes
    print("device RANSAC: worst pose error %.4f m / %.5f rad (restatement %.4f / %.5f)" % (worst_t, worst_R, E_t, E_R))
    assert worst_t <= 3 * E_t and worst_R <= 3 * E_R


@pytest.mark.gpu
def test_pnp_library_draws_from_a_seed():
    s = rl.make_pnp_scene(100)
    a, b, c = (rl.PnPSolver([s], n_rows=ROWS, seed=seed, params=PARAMS) for seed in (5, 5, 6))
    rows = a.rows(0)[0]
    assert rows.min() >= 0 and rows.max() < 60 and all(len(set(r)) == 4 for r in rows.tolist())
    assert np.array_equal(rows, b.rows(0)[0]) and not np.array_equal(rows, c.rows(0)[0])
    assert a.iterate(0, 5).found


@pytest.mark.gpu
def test_pnp_invalid_arguments_touch_nothing():
    s = rl.make_pnp_scene(100)
    cand = rl._Candidate(s["Xw"], s["uv"], s["sigma2"], s["key_index"], s["n_frame_keys"], s["K"])
    rec, par = cand.record(), rl._params_record(PARAMS)
    L = _lib.lib()

    def create(samples, n_rows, params=par):
        h = ctypes.c_void_p(12345)
        rc = L.vieo_pnp_create(ctypes.byref(h), rec.ctypes.data, 1, params.ctypes.data,
                               samples.ctypes.data if samples is not None else None, n_rows, 0)
        return rc, h.value

    assert create(None, 513) == (_lib.VIEO_E_INVALID, None)  # S > 512
    assert create(None, 0) == (_lib.VIEO_E_INVALID, None)
    bad = rl.draw_samples(np.random.default_rng(0), 60, ROWS)
    bad[7, 2] = 60  # out of range
    assert create(bad, ROWS) == (_lib.VIEO_E_INVALID, None)
    bad[7, 2] = bad[7, 0]  # drawn twice
    assert create(bad, ROWS) == (_lib.VIEO_E_INVALID, None)
    five = rl._params_record(dict(PARAMS, min_set=5))
    assert create(None, ROWS, five) == (_lib.VIEO_E_INVALID, None)
    rc, h = create(None, 512)
    assert rc == _lib.VIEO_OK and h
    L.vieo_pnp_destroy(ctypes.c_void_p(h))


def _trace_rows(trace):
    return [(int(v["cand"]), int(v["call"]), int(v["row"]), int(v["no_more"]), int(v["found"]), int(v["n_inliers"]),
             [int(x) for x in v["n_good"]], [int(x) for x in v["n_additional"]]) for v in trace]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["widen", "direct", "none", "narrow"])
def test_relocalize_parity(oracle, kind):
    """vieo_relocalize against the restated chain, which runs with the device's PnPSolver as its PnP (covered by the
    tests above) and with the oracle's optimisations and searches"""
    frame, cands, truth, samples = _chain_case(kind)
    want = ref.relocalize(frame, cands, samples, lambda c, s, p: rl.PnPSolver(c, s, params=p), oracle, PARAMS)
    got = rl.Relocalization(frame, cands, samples)
    assert got["found"] == want["found"] and got["cand"] == want["cand"] and got["n_good"] == want["n_good"]
    assert _trace_rows(got["trace"]) == _trace_rows(want["trace"])
    assert np.array_equal(got["mp_ref"], want["mp_ref"]) and np.array_equal(got["outlier"], want["outlier"] != 0)
    if want["found"]:
        dt, dR = ref.pose_error(got["Tcw"][:3, :3], got["Tcw"][:3, 3], want["Tcw"][:3, :3], want["Tcw"][:3, 3])
        assert dt <= 1e-4 and dR <= 1e-4
        p, q = rl.nav_from_tcw(got["Tcw"], frame.Rcb, frame.tcb)
        assert np.abs(got["nav"]["p"] - p).max() < 1e-5 and min(np.abs(got["nav"]["q"] - q).max(), np.abs(got["nav"]["q"] + q).max()) < 1e-5
    trace = got["trace"]
    if kind == "widen":
        assert got["found"] and _took_widening_search(trace)
    elif kind == "direct":
        assert got["found"] and not _took_widening_search(trace)
    elif kind == "none":
        last = {int(v["cand"]): v for v in trace}
        assert not got["found"] and len(last) == len(cands) and all(v["no_more"] for v in last.values())


@pytest.mark.gpu
def test_relocalize_invalid_arguments_touch_nothing():
    frame, cands, truth, samples = _chain_case("direct")
    rig = rl.RelocFrame(frame.keys, frame.uright, frame.desc, frame.bow.feat_vec, frame.K, frame.bf, frame.scale, n_cams=2)
    for f, kw in ((rig, dict(samples=samples)), (frame, dict(n_rows=513)), (frame, dict(n_rows=0))):
        rc, res, mp_ref, outlier, trace = rl.relocalize_call(f, cands, **kw)
        assert rc == _lib.VIEO_E_INVALID
        assert (mp_ref == -7).all() and (outlier == 7).all() and not res["n_visits"] and not trace["call"].any()
    rc, res, _, _, _ = rl.relocalize_call(frame, cands, n_rows=512, seed=3)  # the library's own draws
    assert rc == _lib.VIEO_OK and res["found"]


# ---------------------------------------------------------------------------------------------------------------------
# GPU: inlier masks of more than one 64-bit word, a partly filled last workgroup of pass A
WORD_CASES = ((200, 4), (201, 9), (203, 60), (204, 64), (205, 65), (206, 128), (207, 129), (208, 130))
WORD_ROWS = 37  # 8 x 37 = 296 pass-A jobs: 18 workgroups of kPnpLanes = 16 and one of 8


@functools.lru_cache(maxsize=None)
def _word_scenes():
    return [(rl.make_pnp_scene(seed, n), rl.draw_samples(np.random.default_rng([seed, 1]), n, WORD_ROWS))
            for seed, n in WORD_CASES]


@functools.lru_cache(maxsize=None)
def _word_batch():
    """the eight candidates in one PnPSolver; (info, rows, records) of each before any iterate"""
    scenes = _word_scenes()
    solver = rl.PnPSolver([s for s, _ in scenes], [smp for _, smp in scenes], params=PARAMS)
    return solver, [(solver.info(c), solver.rows(c), solver.records(c)) for c in range(len(scenes))]


@pytest.mark.gpu
def test_pnp_tables_across_mask_words():
    scenes = _word_scenes()
    solver, taps = _word_batch()
    finite_all = rows_all = 0
    for c, ((seed, n), (s, smp)) in enumerate(zip(WORD_CASES, scenes)):
        info, (samples, Rt, count, mask), (rec_row, rec_Rt, rec_count, rec_mask) = taps[c]
        assert info["n"] == n and info["mask_words"] == (n + 63) // 64 and info["n_rows"] == WORD_ROWS, seed
        assert mask.shape == (WORD_ROWS, n) and rec_mask.shape[1] == n
        if n < info["min_inliers"]:  # N < mRansacMinInliers: no solver, bNoMore at the first call (PnPsolver.cc:161)
            assert info["min_inliers"] == 10 and info["n_records"] == 0, seed
            assert not Rt.any() and not count.any() and not mask.any(), seed
            r = solver.iterate(c, 5)
            assert r.no_more and not r.found and r.Tcw is None and solver.info(c)["iterations"] == 0, seed
            continue
        want = _ref_solver(s, smp).iterate(5)
        assert np.array_equal(samples, smp), seed
        finite, entries, excused = _check_tables(s, Rt, count, mask, "seed %d rows" % seed)
        finite_all, rows_all = finite_all + finite, rows_all + WORD_ROWS
        assert excused <= 0.01 * entries, (seed, excused)
        assert info["n_records"] == len(rec_row) > 0, seed
        f2, e2, x2 = _check_tables(s, rec_Rt, rec_count, rec_mask, "seed %d records" % seed)
        assert f2 == len(rec_row) and x2 <= 0.01 * e2, (seed, f2, x2)
        # the records are the rows that raise the best-so-far count
        best, opened = 0, []
        for r in range(WORD_ROWS):
            if count[r] >= info["min_inliers"] and count[r] > best:
                best = count[r]
                opened.append(r)
        assert rec_row.tolist() == opened, seed
        replay = _replay(solver, c, s)
        got = solver.iterate(c, 5)
        _same(got, replay.iterate(5), seed)
        assert solver.info(c)["iterations"] == replay.iterations
        assert got.found == want.found and got.found, seed
        print("seed %d, n = %d: %d inliers (restatement %d), %d records" % (seed, n, got.n_inliers, want.n_inliers, len(rec_row)))
        assert int(got.inliers.sum()) == got.n_inliers
        if n >= 128:
            assert got.n_inliers > 64 and got.inliers[64:].any() and mask[:, 64:].any() and rec_mask[:, 64:].any(), seed
    assert rows_all == 6 * WORD_ROWS and finite_all > 0.9 * rows_all  # the share test_pnp_hypotheses_table asks for


@pytest.mark.gpu
def test_pnp_batch_independence_across_mask_words():
    """a candidate's tables do not depend on its neighbours in the batch, on its place in the concatenated arrays, or
    on the workgroup its rows fall into; Refine alone on a record's pass-A mask is the record"""
    scenes = _word_scenes()
    _, taps = _word_batch()
    for c, ((seed, n), (s, smp)) in enumerate(zip(WORD_CASES, scenes)):
        info, rows, records = taps[c]
        if n < info["min_inliers"]:
            continue
        alone = rl.PnPSolver([s], [smp], params=PARAMS)
        for a, b in zip(rows + records, alone.rows(0) + alone.records(0)):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), seed
        rec_row, rec_Rt, rec_count, rec_mask = records
        Rt, cnt, out = rl.PnPSolver.refine_masks(s, rows[3][rec_row], PARAMS)
        assert Rt.tobytes() == rec_Rt.tobytes() and np.array_equal(cnt, rec_count) and np.array_equal(out, rec_mask), seed


def _refine_case_wide():
    """one noisy all-inlier scene of 130 correspondences (three mask words) and 60 inlier sets of 6 ... 130 of them"""
    s = rl.make_pnp_scene(77, 130, 0.0, 0.5)
    rng = np.random.default_rng(78)
    masks = np.zeros((60, 130), bool)
    for i in range(60):
        masks[i, rng.choice(130, 6 + (i * 124) // 59, replace=False)] = True
    return s, masks


@pytest.mark.gpu
def test_pnp_refine_parity_across_mask_words():
    s, masks = _refine_case_wide()
    assert masks[0].sum() == 6 and masks[-1].sum() == 130 and masks[:, 64:].any() and masks[:, 128:].any()
    Rt, count, out = rl.PnPSolver.refine_masks(s, masks, PARAMS)
    worst_t = worst_R = 0.0
    for i, m in enumerate(masks):
        idx = np.flatnonzero(m)
        R0, t0 = ref.epnp(s["Xw"][idx].astype(np.float64), s["uv"][idx].astype(np.float64), s["K"])
        dt, dR = ref.pose_error(Rt[i, :9].reshape(3, 3), Rt[i, 9:], R0, t0)
        worst_t, worst_R = max(worst_t, dt), max(worst_R, dR)
    print("pass B vs restated EPnP, n_inl = 6 ... 130 of 130: %.3g m, %.3g rad" % (worst_t, worst_R))
    assert worst_t <= 1e-9 and worst_R <= 1e-9
    finite, entries, excused = _check_tables(s, Rt, count, out, "refine, three words")
    assert finite == len(masks) and excused <= 0.01 * entries
    assert out[:, 64:].any() and out[:, 128:].any()
