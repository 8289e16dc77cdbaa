"""Relocalisation of a lost frame of a camera rig on the device: vieo_search_by_bow_rig, vieo_pnp_create_rig with its
taps, vieo_relocalize_rig against the restatement of tests/reloc_rig_ref.py, which tests/test_relocalization_rig.py
checks on the CPU (scenes, helpers and the CPU figures come from there; its module docstring says why the tests that ask
for the true pose put the map points on the plane z = 1 of their camera), and the rectified PnP instances against the
bytes of the parent commit (tests/golden/pnp_rectified_rows.npz)."""
import os

import numpy as np
import pytest

from tests import reloc_ref as ref
from tests import reloc_rig_ref as rref
from tests import test_relocalization_rig as cpu
from vieo_slam_amd import _lib
from vieo_slam_amd import relocalization as rl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RIGS = cpu.RIGS
PARAMS = cpu.PARAMS
ROWS = cpu.ROWS
DEEP = cpu.DEEP


def _solver(scenes, **kw):
    return rl.PnPSolver([s for s, _ in scenes], [smp for _, smp in scenes], params=PARAMS, rig=scenes[0][0]["rig"]["pnp"], **kw)


@pytest.mark.gpu
def test_search_by_bow_rig_parity():
    for n_cams in (4, 2, 1):
        frame, key_cam, cam_first, kfs = rl.make_bow_rig_scene(1, n_cams)
        for check in (True, False):
            got = rl.SearchByBoWRig(kfs, frame, key_cam, n_cams, 0.75, check)  # all 3 candidates in one call
            twice = 0
            for kf, (match, n) in zip(kfs, got):
                m, n_ref, _ = rref.search_by_bow(kf, frame, key_cam, 0.75, check)
                assert np.array_equal(match, m) and n == n_ref, (n_cams, check)
                held = kf.mp_id[match[match >= 0]]
                twice += len(held) - len(set(held.tolist()))
            assert (twice > 0) == (n_cams > 1)  # a map point in two images: not what the rectified walk gives
            # key_cam all zero (and one camera with a rig record): the rectified entry, byte for byte
            zero = rl.SearchByBoWRig(kfs, frame, np.zeros_like(key_cam), n_cams, 0.75, check)
            for (a, na), (b, nb) in zip(zero, rl.SearchByBoW(kfs, frame, 0.75, check)):
                assert a.tobytes() == b.tobytes() and na == nb
    # a key of an image the frame does not have: refused, nothing written
    frame, key_cam, cam_first, kfs = rl.make_bow_rig_scene(1, 2)
    recs = np.concatenate([k.rec for k in kfs])
    match, n_matches = np.full((3, 300), -7, np.int32), np.full(3, -7, np.int32)
    bad = key_cam.copy()
    bad[17] = 2
    for cams, nc in ((bad, 2), (key_cam, 0), (key_cam, 5)):
        rc = _lib.lib().vieo_search_by_bow_rig(frame.rec.ctypes.data, cams.ctypes.data, nc, recs.ctypes.data, 3, 0.75, 1,
                                               match.ctypes.data, n_matches.ctypes.data)
        assert rc == _lib.VIEO_E_INVALID and (match == -7).all() and (n_matches == -7).all()


@pytest.mark.gpu
def test_pnp_usun():
    """vieo_pnp_tap_usun against the restatement.  The host build of the device arithmetic gives the restatement's
    doubles exactly (CPU figure 0 px, cpu.RIG_CPU_FIGURES), so the bound is the floor: 1e-9 px."""
    bound = max(10 * cpu.RIG_CPU_FIGURES["usun"], 1e-9)
    for rig_kind in RIGS:
        scenes = [cpu.scene_samples(500, rig_kind), cpu.scene_samples(501, rig_kind, DEEP), cpu.scene_samples(502, rig_kind, DEEP, n=65)]
        solver = _solver(scenes)
        worst = 0.0
        for c, (s, _) in enumerate(scenes):
            got = solver.usun(c)
            assert got.shape == (len(s["uv"]), 2) and np.isfinite(got).all()
            worst = max(worst, np.abs(got - rref.usun(s["uv"], s["cam_of"], s["rig"])).max())
        print("%s: usun, device vs restatement: %.3g px" % (rig_kind, worst))
        assert worst <= bound
    flat = rl.PnPSolver([rl.make_pnp_scene(100)], n_rows=4, params=PARAMS)  # a rectified handle has none
    assert _lib.lib().vieo_pnp_tap_usun(flat._h, 0, np.zeros((60, 2)).ctypes.data) == _lib.VIEO_E_INVALID


@pytest.mark.gpu
def test_pnp_rig_refine_parity():
    """pass B on given inlier sets of 6 ... 60 points spread over the cameras against the restated rig EPnP.  The host
    build's CPU figure is 2.5e-11 m / 2.1e-11 rad (unit plane) and 1.5e-13 m / 9.4e-15 rad (1.5-12 m), at most a tenth
    of the rectified test's 1e-9 m / 1e-9 rad, which is therefore the bound."""
    assert max(max(cpu.RIG_CPU_FIGURES["epnp_unit"]), max(cpu.RIG_CPU_FIGURES["epnp_deep"])) <= 1e-10
    for rig_kind in RIGS:
        for plane_z in (cpu.UNIT, DEEP):
            s, masks = cpu.refine_case(rig_kind, plane_z)
            assert all(len(set(s["cam_of"][m].tolist())) > 1 for m in masks)
            Rt, count, out = rl.PnPSolver.refine_masks(s, masks, PARAMS, rig=s["rig"]["pnp"])
            un = rref.usun(s["uv"], s["cam_of"], s["rig"])
            worst_t = worst_R = 0.0
            for i, m in enumerate(masks):
                idx = np.flatnonzero(m)
                R0, t0 = rref.epnp(s["Xw"][idx].astype(np.float64), s["uv"][idx].astype(np.float64), un[idx], s["cam_of"][idx], s["rig"])
                dt, dR = ref.pose_error(Rt[i, :9].reshape(3, 3), Rt[i, 9:], R0, t0)
                worst_t, worst_R = max(worst_t, dt), max(worst_R, dR)
            print("%s, plane_z %s: pass B vs restated rig EPnP, n_inl = 6 ... 60: %.3g m, %.3g rad" % (rig_kind, plane_z, worst_t, worst_R))
            assert worst_t <= 1e-9 and worst_R <= 1e-9
            finite, entries, excused = cpu.check_tables(s, Rt, count, out, "refine")
            assert finite == len(masks) and excused <= 0.01 * entries


@pytest.mark.gpu
def test_pnp_rig_tables():
    """pass A on 8 candidates, 4 per rig kind: every finite row's count and mask are the restated CheckInliers at that
    row's pose (test_relocalization._check_tables's rule and caps; the host build stays inside both on these scenes,
    CPU part).  The first candidate per rig holds a map point twice and its row 0 draws both copies."""
    for rig_kind in RIGS:
        scenes = cpu.table_scenes(rig_kind)
        s0, smp0 = scenes[0]
        assert np.array_equal(s0["Xw"][0], s0["Xw"][1]) and s0["cam_of"][0] != s0["cam_of"][1] and {0, 1} <= set(smp0[0].tolist())
        solver = _solver(scenes)
        finite = entries = excused = 0
        for c, (s, smp) in enumerate(scenes):
            info = solver.info(c)
            assert (info["min_inliers"], info["max_its"], info["n_rows"], info["mask_words"]) == (30, 35, ROWS, 1)
            samples, Rt, count, mask = solver.rows(c)
            assert np.array_equal(samples, smp)
            f, e, x = cpu.check_tables(s, Rt, count, mask, "%s candidate %d" % (rig_kind, c))
            finite, entries, excused = finite + f, entries + e, excused + x
        print("%s pass A: %d of %d rows finite, %d of %d entries next to the threshold" % (rig_kind, finite, 4 * ROWS, excused, entries))
        assert finite > 0.9 * 4 * ROWS and excused <= 0.01 * entries


@pytest.mark.gpu
def test_pnp_rig_behind_camera():
    """the pose Refine finds on the correspondences of camera 0 alone, in a scene whose other correspondences were moved
    behind their cameras (the map point mirrored through the camera's centre) or onto the plane z = 0 of their camera:
    their flags are the restatement's -- outliers, whatever Project makes of them -- and the count is finite"""
    for rig_kind in RIGS:
        s = rl.make_pnp_rig_scene(600, rig_kind, 60, 0.0, 0.5, plane_z=cpu.UNIT)
        rig = s["rig"]
        Xw = s["Xw"].astype(np.float64)
        moved = np.flatnonzero(s["cam_of"] != 0)
        for k, i in enumerate(moved):
            c = s["cam_of"][i]
            Pc = rig["Tcr_a"][c][:, :3] @ s["Pr"][i] + rig["Tcr_a"][c][:, 3]
            Pc = -Pc if k % 2 else Pc * np.array([1.0, 1.0, 0.0])  # behind the camera / z = 0
            Pr = rig["Trc_a"][c][:, :3] @ Pc + rig["Trc_a"][c][:, 3]
            Xw[i] = s["R"].T @ (Pr - s["t"])
        s = dict(s, Xw=Xw.astype(np.float32))
        masks = np.stack([s["cam_of"] == 0, s["cam_of"] == 0])
        masks[1, np.flatnonzero(masks[1])[0]] = False
        Rt, count, out = rl.PnPSolver.refine_masks(s, masks, PARAMS, rig=rig["pnp"])
        max_err = ref.max_error(s["sigma2"], PARAMS["th2"])
        for r in range(2):
            assert np.isfinite(Rt[r]).all() and max(ref.pose_error(Rt[r, :9].reshape(3, 3), Rt[r, 9:], s["R"], s["t"])) < 0.05
            R, t = Rt[r, :9].reshape(3, 3), Rt[r, 9:]
            want = rref.check_inliers(R, t, s["Xw"], s["uv"], max_err, s["cam_of"], rig)
            e = rref.getuv(R, t, s["Xw"], s["cam_of"], rig)
            assert np.array_equal(out[r], want) and count[r] == want.sum() and not want[moved].any()
            assert want[s["cam_of"] == 0].sum() >= 0.8 * (s["cam_of"] == 0).sum()
            Pz = [(rig["Tcr_a"][s["cam_of"][i]] @ np.append(R @ s["Xw"][i].astype(np.float64) + t, 1.0))[2] for i in moved]
            assert min(Pz) < -0.5 and np.abs(Pz).min() < 0.05  # some behind, some next to z = 0
            print("%s: %d moved correspondences, %d with a pixel that is not finite, count %d" % (
                rig_kind, len(moved), int((~np.isfinite(e[moved])).any(axis=1).sum()), count[r]))


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
def test_pnp_rig_iterate_is_the_replay_of_its_tables():
    for rig_kind in RIGS:
        scenes = [cpu.scene_samples(seed, rig_kind) for seed in cpu.SEEDS]
        scenes += [cpu.scene_samples(seed, rig_kind, DEEP) for seed in cpu.SEEDS[:4]]  # (mostly without a pose: bNoMore)
        junk = rl.make_pnp_rig_scene(99, rig_kind, 20, 1.0, 0.5)
        scenes.append((junk, rl.draw_samples(np.random.default_rng(5), 20, ROWS)))
        solver = _solver(scenes)
        for c, (s, _) in enumerate(scenes[:-1]):
            replay = _replay(solver, c, s)
            for call in range(3):
                _same(solver.iterate(c, 5), replay.iterate(5), (rig_kind, c, call))
            assert solver.info(c)["iterations"] == replay.iterations
        c = len(scenes) - 1
        r = solver.iterate(c, 5)
        _same(r, _replay(solver, c, junk).iterate(5), "junk")
        assert r.no_more and not r.found and solver.info(c)["iterations"] == 35


@pytest.mark.gpu
def test_pnp_rig_outcome():
    for rig_kind in RIGS:
        E_t, E_R = cpu.worst_restated_error(rig_kind)
        scenes = [cpu.scene_samples(seed, rig_kind) for seed in cpu.SEEDS]
        runs = []
        for _ in range(2):
            solver = _solver(scenes)
            runs.append([(solver.iterate(c, 5), solver.rows(c), solver.records(c), solver.usun(c)) for c in range(len(scenes))])
        worst_t = worst_R = 0.0
        for c, (s, _) in enumerate(scenes):
            r = runs[0][c][0]
            assert r.found and r.n_inliers > 30, (rig_kind, cpu.SEEDS[c])
            dt, dR = ref.pose_error(r.Tcw[:3, :3], r.Tcw[:3, 3], s["R"], s["t"])
            worst_t, worst_R = max(worst_t, dt), max(worst_R, dR)
            _same(r, runs[1][c][0], cpu.SEEDS[c])
            for a, b in zip(runs[0][c][1] + runs[0][c][2] + (runs[0][c][3],), runs[1][c][1] + runs[1][c][2] + (runs[1][c][3],)):
                assert a.tobytes() == b.tobytes(), cpu.SEEDS[c]  # two runs on the same inputs: the same bytes
        print("%s: device rig RANSAC, worst pose error %.4f m / %.5f rad (restatement %.4f / %.5f)" % (rig_kind, worst_t, worst_R, E_t, E_R))
        assert worst_t <= 3 * E_t and worst_R <= 3 * E_R


@pytest.mark.gpu
def test_pnp_rig_across_mask_words():
    """n = 64, 65, 129: one, two and three mask words; 37 rows: 3 x 37 = 111 pass-A jobs, six workgroups of 16 and one of 15"""
    for rig_kind in RIGS:
        scenes = [cpu.scene_samples(700 + n, rig_kind, n=n, rows=37) for n in (64, 65, 129)]
        solver = _solver(scenes)
        for c, (s, smp) in enumerate(scenes):
            n = len(s["Xw"])
            info = solver.info(c)
            assert info["n"] == n and info["mask_words"] == (n + 63) // 64 and info["n_rows"] == 37
            samples, Rt, count, mask = solver.rows(c)
            rec_row, rec_Rt, rec_count, rec_mask = solver.records(c)
            assert np.array_equal(samples, smp) and mask.shape == (37, n) and info["n_records"] == len(rec_row) > 0
            finite, entries, excused = cpu.check_tables(s, Rt, count, mask, "%s n = %d rows" % (rig_kind, n))
            assert finite > 0.9 * 37 and excused <= 0.01 * entries
            f2, e2, x2 = cpu.check_tables(s, rec_Rt, rec_count, rec_mask, "%s n = %d records" % (rig_kind, n))
            assert f2 == len(rec_row) and x2 <= 0.01 * e2
            alone = rl.PnPSolver([s], [smp], params=PARAMS, rig=s["rig"]["pnp"])  # the batch does not matter
            for a, b in zip(solver.rows(c) + solver.records(c), alone.rows(0) + alone.records(0)):
                assert a.tobytes() == b.tobytes(), (rig_kind, n)
            replay = _replay(solver, c, s)
            got = solver.iterate(c, 5)
            _same(got, replay.iterate(5), (rig_kind, n))
            assert got.found and int(got.inliers.sum()) == got.n_inliers
            if n > 64:
                assert mask[:, 64:].any()
            if n >= 128:
                assert rec_mask[:, 64:].any() and got.inliers[64:].any()


@pytest.mark.gpu
def test_rectified_pnp_unchanged():
    """vieo_pnp_create on the rectified seeds: the row and record bytes of the parent commit (SHA-256 per seed, written
    there by tests/golden/make_pnp_rectified_golden.py)"""
    from tests.golden import make_pnp_rectified_golden as gold
    want = np.load(os.path.join(ROOT, "tests", "golden", "pnp_rectified_rows.npz"))
    assert want["seeds"].tolist() == gold.SEEDS and int(want["n_rows"]) == gold.ROWS
    rows, records = gold.digests()
    for i, seed in enumerate(gold.SEEDS):
        assert rows[i].tobytes() == want["rows_sha256"][i].tobytes(), seed
        assert records[i].tobytes() == want["records_sha256"][i].tobytes(), seed


def _trace_rows(trace):
    return [(int(v["cand"]), int(v["call"]), int(v["row"]), int(v["no_more"]), int(v["found"]), int(v["n_inliers"]),
             [int(x) for x in v["n_good"]], [int(x) for x in v["n_additional"]]) for v in trace]


@pytest.mark.gpu
@pytest.mark.parametrize("rig_kind", RIGS)
@pytest.mark.parametrize("kind", ["widen", "direct", "none", "deep"])
def test_relocalize_rig_parity(oracle, kind, rig_kind):
    """vieo_relocalize_rig against the restated chain, which runs with the device's rig PnP as its PnP (covered by the
    tests above) and with the oracle's rig optimisation and searches.  "deep": map points 1.5-12 m away, where usun carries
    the baselines' parallax; parity is asked for, whatever the chain makes of it"""
    frame, rig, cands, truth, samples = cpu.chain_case(kind, rig_kind)
    make = lambda c, s, p: rl.PnPSolver(c, s, params=p, rig=rig.pnp)  # noqa: E731
    want = rref.relocalize(frame, rig, cands, samples, make, oracle, PARAMS)
    got = rl.RelocalizationRig(frame, rig, cands, samples)
    assert got["found"] == want["found"] and got["cand"] == want["cand"] and got["n_good"] == want["n_good"]
    assert _trace_rows(got["trace"]) == _trace_rows(want["trace"])
    assert np.array_equal(got["mp_ref"], want["mp_ref"]) and np.array_equal(got["outlier"], want["outlier"] != 0)
    if want["found"]:
        dt, dR = ref.pose_error(got["Tcw"][:3, :3], got["Tcw"][:3, 3], want["Tcw"][:3, :3], want["Tcw"][:3, 3])
        assert dt <= 1e-4 and dR <= 1e-4
        p, q = rl.nav_from_tcw(got["Tcw"], frame.Rcb, frame.tcb)
        assert np.abs(got["nav"]["p"] - p).max() < 1e-5 and min(np.abs(got["nav"]["q"] - q).max(), np.abs(got["nav"]["q"] + q).max()) < 1e-5
        held = got["mp_ref"] >= 0
        assert kind == "deep" or len(set(rig.key_cam()[held].tolist())) >= 2  # the winner holds keys of at least two cameras
    trace = got["trace"]
    if kind == "widen":
        assert got["found"] and cpu.took_widening_search(trace)
    elif kind == "direct":
        assert got["found"] and not cpu.took_widening_search(trace)
    elif kind == "none":
        last = {int(v["cand"]): v for v in trace}
        assert not got["found"] and len(last) == len(cands) and all(v["no_more"] for v in last.values())


@pytest.mark.gpu
def test_relocalize_rig_invalid_arguments_touch_nothing():
    frame, rig, cands, truth, samples = cpu.chain_case("direct", "radtan2")

    def variant(n_cams=None, cam_first=None, sbp=True):
        pnp = rig.pnp.copy()
        if n_cams is not None:
            pnp["n_cams"] = n_cams
        return rl.RelocRig(pnp, rig.cam_first if cam_first is None else cam_first, rig.sbp if sbp else None, rig.pose_cams)

    down = rig.cam_first.copy()
    down[1] = down[2] + 1  # camera 0 would end behind the frame's last key: decreasing
    cases = [(variant(n_cams=0), dict(samples=samples)), (variant(n_cams=5), dict(samples=samples)),
             (variant(cam_first=down), dict(samples=samples)), (variant(sbp=False), dict(samples=samples)),
             (rig, dict(n_rows=0)), (rig, dict(n_rows=513))]
    for r, kw in cases:
        rc, res, mp_ref, outlier, trace = rl.relocalize_rig_call(frame, r, cands, **kw)
        assert rc == _lib.VIEO_E_INVALID
        assert (mp_ref == -7).all() and (outlier == 7).all() and not res["n_visits"] and not trace["call"].any()
    rc, res, _, _, _ = rl.relocalize_rig_call(frame, rig, cands, n_rows=512, seed=3)  # the library's own draws
    assert rc == _lib.VIEO_OK and res["found"]
    assert max(ref.pose_error(res["Tcw"].reshape(4, 4)[:3, :3], res["Tcw"].reshape(4, 4)[:3, 3], truth["R"], truth["t"])) < 0.02
