"""Relocalisation of a lost frame of a camera rig (Frame::usedistort_, F.mapn2in_ filled), CPU part: the restatement of
tests/reloc_rig_ref.py against independent statements -- a brute-force SearchByBoW, the truth of generated scenes, the
device's rig arithmetic compiled for the host (tests/emul/pnp_rig_emul.cc) -- and the restated chain on the oracle's
rig back ends.  The GPU part is tests/test_relocalization_rig_abi.py, whose bounds rest on the figures printed here.

What the reference's rig PnP is, and what the scenes therefore are.  add_correspondence un-projects a key to the plane
z = 1 of its own camera and moves THAT point into the reference camera with GetTrc(); it is the map point's central
projection there only if the map point lies on that plane (or the camera sits at the reference camera's centre).  A
camera at a baseline b leaves usun a parallax of about fx b |1 - 1/z| pixels: up to 46 px on the two-camera Radtan rig
(b = 0.11 m) and 94 px on the four-camera KB8 rig (whose side cameras look 0.35 rad aside, where the reference camera's
pinhole pixel magnifies it) for map points 1.5-12 m away, where CheckInliers, which projects exactly, then rejects nearly every hypothesis that has a correspondence outside camera 0 (restated RANSAC on seeds
300 ... 305, 40 rows: a pose on 1 of 6 Radtan scenes, 0 of 6 KB8 scenes).  That is the reference's arithmetic and the
library's; what can be asked of it is parity everywhere, and the truth only where the formula is exact.  So the tests
that ask for the true pose (EPnP, RANSAC outcome, the chain) use scenes whose map points lie on the plane z = 1 of the
camera that sees them (plane_z = 1 of the generators), and the parity tests use both kinds.

Figures of the host build of the rig instances (tests/emul/pnp_rig_emul.cc) against the restatement, CPU, both rigs, as
printed by test_device_rig_arithmetic_on_the_host_against_the_restatement: see RIG_CPU_FIGURES below; the GPU bounds
are derived from that dict."""
import ctypes
import functools
import os
import subprocess

import numpy as np

from tests import reloc_ref as ref
from tests import reloc_rig_ref as rref
from vieo_slam_amd import relocalization as rl
from vieo_slam_amd import synth_ba

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RIGS = ("radtan2", "kb8x4")
PARAMS = rl.RELOC_PNP_PARAMS
ROWS = 40
SEEDS = list(range(300, 308))
UNIT, DEEP = 1.0, None  # plane_z of the generators.  UNIT: the map points on the plane z = 1 of their camera: the reference's usun is exact there; DEEP: 1.5-12 m away

# Host build against the restatement, worst over both rigs (printed by the host-build test below, which also asserts
# that a fresh measurement stays within a factor 10 of these): usun in pixels; EPnP for n = 6 ... 60 in metres /
# radians on the unit-plane refine case and on the one with map points 1.5-12 m away.
RIG_CPU_FIGURES = dict(usun=0.0, epnp_unit=(2.5e-11, 2.1e-11), epnp_deep=(1.5e-13, 9.4e-15))


def scene_samples(seed, rig_kind, plane_z=UNIT, n=60, rows=ROWS, **kw):
    s = rl.make_pnp_rig_scene(seed, rig_kind, n, plane_z=plane_z, **kw)
    return s, rl.draw_samples(np.random.default_rng([seed, 1]), n, rows)


def refine_case(rig_kind, plane_z=UNIT):
    """one noisy all-inlier scene of 60 correspondences and 60 inlier sets of 6 ... 60 of them, spread over the cameras"""
    s = rl.make_pnp_rig_scene(77, rig_kind, 60, 0.0, 0.5, plane_z=plane_z)
    rng = np.random.default_rng(78)
    masks = np.zeros((60, 60), bool)
    for i in range(60):
        masks[i, rng.choice(60, 6 + (i * 54) // 59, replace=False)] = True
    return s, masks


@functools.lru_cache(maxsize=None)
def ransac_restated(rig_kind):
    """the restated rig RANSAC on every seed, once: [(first iterate(5), pose error against the truth)]"""
    out = []
    for seed in SEEDS:
        s, samples = scene_samples(seed, rig_kind)
        r = rref.tables(s, samples, PARAMS)[0].iterate(5)
        out.append((r, ref.pose_error(r.Tcw[:3, :3], r.Tcw[:3, 3], s["R"], s["t"]) if r.found else (np.inf, np.inf)))
    return out


def worst_restated_error(rig_kind):
    errs = [e for _, e in ransac_restated(rig_kind)]
    return max(e[0] for e in errs), max(e[1] for e in errs)


@functools.lru_cache(maxsize=None)
def chain_case(kind, rig_kind):
    """a rig relocalisation scene and its sample tables (48 rows per candidate, indices below its BoW matches).  "deep"
    is the "direct" plan with the map points 1.5-12 m away, where the reference's usun carries the baselines' parallax"""
    seed = {"widen": 1, "direct": 2, "none": 3, "deep": 4}[kind]
    frame, rig, cands, truth = rl.make_reloc_rig_scene(seed, "direct" if kind == "deep" else kind, rig_kind,
                                                       plane_z=DEEP if kind == "deep" else UNIT)
    n = [int((rref.search_by_bow(c.bow, frame.bow, rig.key_cam(), 0.75, True)[0] >= 0).sum()) for c in cands]
    samples = [rl.draw_samples(np.random.default_rng([seed, i]), max(k, 4), 48) for i, k in enumerate(n)]
    return frame, rig, cands, truth, samples


def took_widening_search(trace):
    return any(v["n_additional"][0] >= 0 for v in trace)


# ---------------------------------------------------------------------------------------------------------------------
def test_restated_rig_search_by_bow_against_brute_force():
    """per-image best / second best against a statement without the walk over nodes.  Three cameras carry keys, one has
    none; map points are matched in two and in three images; frame keys are equally good for two key-frame keys."""
    frame, key_cam, cam_first, kfs = rl.make_bow_rig_scene(1, 4)
    assert np.diff(cam_first).tolist().count(0) == 1 and len(frame.keys) == 300
    total = dict(skipped=0, ratio=0, replaced=0, kept=0, rotation=0, empty_slot=0, second_image=0)
    in_two = in_three = 0
    for kf in kfs:
        for check in (True, False):
            m, n, ev = rref.search_by_bow(kf, frame, key_cam, 0.75, check)
            m2, n2 = rref.search_by_bow_brute(kf, frame, key_cam, 0.75, check)
            assert np.array_equal(m, m2) and n == n2
            assert n == int((m >= 0).sum()) > 40
            held = kf.mp_id[m[m >= 0]]
            pairs = set(zip(held.tolist(), key_cam[m >= 0].tolist()))
            assert (held >= 0).all() and len(pairs) == len(held)  # a map point is matched once per image
            images = np.bincount(np.unique(held, return_inverse=True)[1])
            in_two, in_three = in_two + int((images == 2).sum()), in_three + int((images == 3).sum())
            for k in total:
                total[k] += ev[k]
            # the rectified walk cannot give this: with every key in image 0 a map point is matched once
            m0, n0, _ = rref.search_by_bow(kf, frame, np.zeros_like(key_cam), 0.75, check)
            r0, rn0, _ = ref.search_by_bow(kf, frame, 0.75, check)
            assert np.array_equal(m0, r0) and n0 == rn0 and not np.array_equal(m0, m)
    print("map points matched in two images: %d, in three: %d; %s" % (in_two, in_three, total))
    assert in_two > 0 and in_three > 0
    assert all(total[k] > 0 for k in ("skipped", "ratio", "replaced", "rotation", "empty_slot", "second_image")), total


def _usun_bound(s):
    """Per correspondence, in pixels of the reference camera: the un-projection stops at precision_ = 1e-8f on the
    distorted normalised plane (1e-8 f pixels of its own camera), its input is a float pixel (one ulp), and Radtan hands
    its result on as floats (2^-24 relative on the normalised plane).  The first two are errors in the key's own image and
    reach usun through the exact map pixel -> plane z = 1 -> reference camera -> K0, whose Jacobian is taken here by
    central differences of the forward functions; for an undistorted reference-camera key that is the issue's
    precision_ * fx plus the float pixel."""
    rig, h = s["rig"], 1e-6
    fx, fy, cx, cy = s["K"]
    out = np.zeros(len(s["uv"]))
    for i, c in enumerate(s["cam_of"]):
        Trc, Tcr = rig["Trc_a"][c], rig["Tcr_a"][c]
        Pc = Tcr[:, :3] @ s["Pr"][i] + Tcr[:, 3]
        xy = Pc[:2] / Pc[2]

        def pixel(q):
            return np.array(synth_ba.project_camera(rig["cams"][c], (q[0], q[1], 1.0)))

        def reference(q):
            P = Trc[:, :3] @ np.array([q[0], q[1], 1.0]) + Trc[:, 3]
            return np.array([fx * P[0] / P[2] + cx, fy * P[1] / P[2] + cy])

        J_fwd = np.stack([(pixel(xy + d) - pixel(xy - d)) / (2 * h) for d in (np.array([h, 0]), np.array([0, h]))], axis=1)
        J_ref = np.stack([(reference(xy + d) - reference(xy - d)) / (2 * h) for d in (np.array([h, 0]), np.array([0, h]))], axis=1)
        in_image = float(np.spacing(np.float32(np.abs(s["uv"][i]).max()))) + rref.PRECISION * float(rig["cams"][c]["fx"])
        out[i] = (np.linalg.norm(J_ref @ np.linalg.inv(J_fwd), 2) * in_image +
                  np.linalg.norm(J_ref, 2) * 2.0 ** -24 * max(1.0, np.abs(xy).max()))
    return out


def test_restated_usun_is_the_pinhole_projection_in_the_reference_camera():
    """un-project, Trc, K0 of noise-free projections of known points on the plane z = 1 of their camera (module
    docstring) is the point's pinhole projection in the reference camera, to _usun_bound.  Off that plane it is not: the
    parallax of the baseline is printed."""
    for rig_kind in RIGS:
        s = rl.make_pnp_rig_scene(5, rig_kind, 120, 0.0, 0.0, plane_z=UNIT)
        fx, fy, cx, cy = s["K"]
        want = np.stack([fx * s["Pr"][:, 0] / s["Pr"][:, 2] + cx, fy * s["Pr"][:, 1] / s["Pr"][:, 2] + cy], axis=1)
        err = np.abs(rref.usun(s["uv"], s["cam_of"], s["rig"]) - want).max(axis=1)
        bound = _usun_bound(s)
        deep = rl.make_pnp_rig_scene(5, rig_kind, 120, 0.0, 0.0)
        want_deep = np.stack([fx * deep["Pr"][:, 0] / deep["Pr"][:, 2] + cx, fy * deep["Pr"][:, 1] / deep["Pr"][:, 2] + cy], axis=1)
        parallax = np.abs(rref.usun(deep["uv"], deep["cam_of"], deep["rig"]) - want_deep).max(axis=1)
        print("%s: usun against the pinhole projection, worst %.3g px (its bound %.3g, worst ratio %.3g; reference camera "
              "alone: %.3g px against precision * fx + ulp = %.3g); 1.5-12 m away: %.3g px in camera 0, %.3g px elsewhere"
              % (rig_kind, err.max(), bound[np.argmax(err)], (err / bound).max(), err[s["cam_of"] == 0].max(),
                 bound[s["cam_of"] == 0].max(), parallax[deep["cam_of"] == 0].max(), parallax[deep["cam_of"] != 0].max()))
        assert (err <= bound).all()
        assert parallax[deep["cam_of"] == 0].max() <= bound.max() and parallax[deep["cam_of"] != 0].max() > 1.0


def test_restated_rig_epnp_recovers_the_true_pose():
    """all-inlier noise-free sets of n >= 6 spread over all cameras, the map points on the plane z = 1 of their camera
    (module docstring).  The bound is test_restated_epnp_recovers_the_true_pose's 1e-4; the usun precision (1e-4 px at
    the worst) does not ask for more."""
    for rig_kind in RIGS:
        rng = np.random.default_rng(11)
        worst = 0.0
        for n in (6, 8, 20, 60):
            for _ in range(25):
                s = rl.make_pnp_rig_scene(0, rig_kind, n, 0.0, 0.0, rng=rng, plane_z=UNIT)
                assert len(set(s["cam_of"].tolist())) == len(s["rig"]["cams"])
                un = rref.usun(s["uv"], s["cam_of"], s["rig"])
                R, t = rref.epnp(s["Xw"].astype(np.float64), s["uv"].astype(np.float64), un, s["cam_of"], s["rig"])
                worst = max(worst, *ref.pose_error(R, t, s["R"], s["t"]))
        print("%s: worst error of the restated rig EPnP on noise-free sets: %.3g" % (rig_kind, worst))
        assert worst <= 1e-4


def test_restated_rig_ransac_returns_a_pose_on_every_seed():
    for rig_kind in RIGS:
        runs = ransac_restated(rig_kind)
        assert all(r.found for r, _ in runs), rig_kind
        E_t, E_R = worst_restated_error(rig_kind)
        print("%s: restated rig RANSAC, worst pose error %.4f m / %.5f rad, latest first success at row %d"
              % (rig_kind, E_t, E_R, max(r.row for r, _ in runs)))
        assert E_t < 0.5 and E_R < 0.5  # (map points 1 m away seen under 0.5 px of noise, 4-point and refined poses)


@functools.lru_cache(maxsize=None)
def emul():
    """tests/emul/pnp_rig_emul.cc: the rig instances' lane functions (csrc/pnp_device.h, pnp_usun.h) compiled for the host"""
    out = os.path.join(ROOT, "tests", "emul", "libpnp_rig_emul.so")
    csrc = os.path.join(ROOT, "vieo_slam_amd", "csrc")
    deps = [os.path.join(ROOT, "tests", "emul", "pnp_rig_emul.cc")] + [os.path.join(csrc, h) for h in (
        "pnp_device.h", "pnp_usun.h", "cam_project.h", "cam_unproject.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", out, deps[0], "-lm"])
    L = ctypes.CDLL(out)
    for f in (L.emul_pnp_rig_usun, L.emul_pnp_rig_epnp, L.emul_pnp_rig_check):
        f.restype = ctypes.c_int
    P = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731

    def usun(s):
        uv, cam, K = np.ascontiguousarray(s["uv"], np.float32), np.ascontiguousarray(s["cam_of"], np.uint8), np.array(s["K"], np.float32)
        out = np.zeros((len(uv), 2))
        assert L.emul_pnp_rig_usun(P(s["rig"]["pnp"]), P(uv), P(cam), len(uv), P(K), P(out)) == 0
        return out

    def epnp(s, idx):
        Xw, uv = np.ascontiguousarray(s["Xw"], np.float32), np.ascontiguousarray(s["uv"], np.float32)
        cam, K, idx, Rt = np.ascontiguousarray(s["cam_of"], np.uint8), np.array(s["K"], np.float32), np.ascontiguousarray(idx, np.int32), np.zeros(12)
        assert L.emul_pnp_rig_epnp(P(s["rig"]["pnp"]), P(Xw), P(uv), P(cam), len(Xw), P(K), P(idx), len(idx), P(Rt)) == 0
        return Rt[:9].reshape(3, 3).copy(), Rt[9:].copy()

    def check(s, R, t, max_err):
        Xw, uv, me = (np.ascontiguousarray(a, np.float32) for a in (s["Xw"], s["uv"], max_err))
        cam, K = np.ascontiguousarray(s["cam_of"], np.uint8), np.array(s["K"], np.float32)
        Rt = np.concatenate([np.asarray(R, np.float64).reshape(-1), np.asarray(t, np.float64)])
        words = np.zeros((1, (len(Xw) + 63) // 64), np.uint64)
        n = L.emul_pnp_rig_check(P(s["rig"]["pnp"]), P(Xw), P(uv), P(cam), P(me), len(Xw), P(K), P(Rt), P(words))
        return n, rl._unpack_masks(words, len(Xw))[0]

    return usun, epnp, check


def host_tables(s, samples):
    """reloc_rig_ref.tables with the host build's EPnP / CheckInliers in place of the restated ones"""
    _, epnp, check = emul()
    max_err = ref.max_error(s["sigma2"], PARAMS["th2"])
    return rref.tables(s, samples, PARAMS, solver=lambda idx: epnp(s, idx), check=lambda R, t: check(s, R, t, max_err)[1])


def check_tables(s, Rt, count, mask, what):
    """test_relocalization._check_tables for a rig scene: the mask is the restated rig CheckInliers at the row's own
    pose except within 1e-4 relative of the threshold; returns (finite rows, entries, excused)"""
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
            e2 = rref.reprojection_error2(R, t, s["Xw"], s["uv"], s["cam_of"], s["rig"])
            near = np.abs(e2.astype(np.float64) / max_err.astype(np.float64) - 1.0) < 1e-4
        differ = mask[r] != (e2 < max_err)
        assert not (differ & ~near).any(), (what, r, np.flatnonzero(differ & ~near))
        entries += len(e2)
        excused += int(near.sum())
    return finite, entries, excused


def table_scenes(rig_kind):
    """the four candidates per rig of the pass-A table test: two unit-plane scenes, two with map points 1.5-12 m away;
    the first holds a map point twice (correspondences 0 and 1) and its sample row 0 draws both copies"""
    out = []
    for k, (seed, plane_z) in enumerate(((400, UNIT), (401, UNIT), (402, DEEP), (403, DEEP))):
        s, smp = scene_samples(seed, rig_kind, plane_z, held_twice=1 if k == 0 else 0)
        if k == 0:
            smp[0] = [0, 1, 7, 12]
        out.append((s, smp))
    return out


def test_device_rig_arithmetic_on_the_host_against_the_restatement():
    """the rig instances' lane functions as plain C++: usun, EPnP for n = 6 ... 60 and CheckInliers against the
    restatement on both rigs, the RANSAC outcome, and the caps of the GPU table test on its scenes"""
    usun, epnp, check = emul()
    fig = dict(usun=0.0, epnp_unit=[0.0, 0.0], epnp_deep=[0.0, 0.0])
    for rig_kind in RIGS:
        for name, plane_z in (("epnp_unit", UNIT), ("epnp_deep", DEEP)):
            s, masks = refine_case(rig_kind, plane_z)
            un = rref.usun(s["uv"], s["cam_of"], s["rig"])
            fig["usun"] = max(fig["usun"], np.abs(usun(s) - un).max())
            max_err = ref.max_error(s["sigma2"], PARAMS["th2"])
            for m in masks:
                idx = np.flatnonzero(m)
                R, t = epnp(s, idx)
                R0, t0 = rref.epnp(s["Xw"][idx].astype(np.float64), s["uv"][idx].astype(np.float64), un[idx], s["cam_of"][idx], s["rig"])
                dt, dR = ref.pose_error(R, t, R0, t0)
                fig[name] = [max(fig[name][0], dt), max(fig[name][1], dR)]
                assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-9 and np.linalg.det(R) > 0
                n, mask = check(s, R, t, max_err)
                assert np.array_equal(mask, rref.check_inliers(R, t, s["Xw"], s["uv"], max_err, s["cam_of"], s["rig"])) and n == mask.sum()
        E_t, E_R = worst_restated_error(rig_kind)
        for seed in SEEDS[:4]:
            s, samples = scene_samples(seed, rig_kind)
            r = host_tables(s, samples)[0].iterate(5)
            assert r.found
            dt, dR = ref.pose_error(r.Tcw[:3, :3], r.Tcw[:3, 3], s["R"], s["t"])
            assert dt <= 3 * E_t and dR <= 3 * E_R
        finite = entries = excused = 0
        for k, (s, smp) in enumerate(table_scenes(rig_kind)):
            _, Rt, count, mask, _ = host_tables(s, smp)
            f, e, x = check_tables(s, Rt, count, mask, "%s scene %d" % (rig_kind, k))
            finite, entries, excused = finite + f, entries + e, excused + x
        print("%s: host build of pass A on the table scenes: %d of %d rows finite, %d of %d entries next to the threshold"
              % (rig_kind, finite, 4 * ROWS, excused, entries))
        assert finite > 0.9 * 4 * ROWS and excused <= 0.01 * entries
    print("host build of the rig instances vs restatement: usun %.3g px; EPnP n = 6 ... 60: unit plane %.3g m / %.3g rad, "
          "1.5-12 m %.3g m / %.3g rad" % (fig["usun"], *fig["epnp_unit"], *fig["epnp_deep"]))
    assert fig["usun"] <= max(10 * RIG_CPU_FIGURES["usun"], 1e-9)
    for name in ("epnp_unit", "epnp_deep"):
        assert fig[name][0] <= 10 * RIG_CPU_FIGURES[name][0] and fig[name][1] <= 10 * RIG_CPU_FIGURES[name][1], (name, fig[name])


def test_a_projection_that_is_not_finite_is_an_outlier_on_the_host():
    """the identity pose and map points on the plane z = 0 of camera 0, on its axis, and behind it: Radtan divides by
    zero, KB8 takes its pinhole branch on the axis (r below 1e-5) and divides by zero there; flags and count are the
    restatement's, and the good correspondences still count.  (A point mirrored through a Radtan camera's centre has the
    pixel of its mirror image: Project does not look at the sign of z, so it stays an inlier there as in the reference.)"""
    _, _, check = emul()
    for rig_kind in RIGS:
        s = rl.make_pnp_rig_scene(610, rig_kind, 24, 0.0, 0.0, plane_z=UNIT)
        Xw = s["Pr"].copy()  # identity pose: the world is the reference camera
        cam0 = np.flatnonzero(s["cam_of"] == 0)
        Xw[cam0[0]] = [0.3, -0.2, 0.0]
        Xw[cam0[1]] = [0.0, 0.0, 0.0]
        Xw[cam0[2]] = -Xw[cam0[2]]
        s = dict(s, Xw=Xw.astype(np.float32))
        max_err = ref.max_error(s["sigma2"], PARAMS["th2"])
        R, t = np.eye(3), np.zeros(3)
        n, mask = check(s, R, t, max_err)
        want = rref.check_inliers(R, t, s["Xw"], s["uv"], max_err, s["cam_of"], s["rig"])
        e = rref.getuv(R, t, s["Xw"], s["cam_of"], s["rig"])
        assert not np.isfinite(e[cam0[:2]]).all() and np.array_equal(mask, want) and n == want.sum() >= len(Xw) - 3, rig_kind
        assert not mask[cam0[:2]].any() and mask[s["cam_of"] != 0].all()


def test_restated_rig_chain(oracle):
    """the restated chain with the restated rig PnP on the oracle's rig optimisation and searches"""
    for rig_kind in RIGS:
        make = lambda c, s, p: rref.RefRigPnPBatch(c, s, p, rl.rig_of(rig_kind))  # noqa: E731
        frame, rig, cands, truth, samples = chain_case("widen", rig_kind)
        out = rref.relocalize(frame, rig, cands, samples, make, oracle, PARAMS)
        assert out["found"] and out["cand"] == 0 and out["n_good"] >= 50 and took_widening_search(out["trace"]), rig_kind
        assert max(ref.pose_error(out["Tcw"][:3, :3], out["Tcw"][:3, 3], truth["R"], truth["t"])) < 0.02
        held = out["mp_ref"] >= 0
        assert len(set(rig.key_cam()[held].tolist())) >= 2 and not out["outlier"][held].any()
        ids = cands[0].bow.mp_id[out["mp_ref"][held]]
        assert len(set(ids.tolist())) < len(ids)  # a map point held by keys of two cameras
        frame, rig, cands, truth, samples = chain_case("direct", rig_kind)
        out = rref.relocalize(frame, rig, cands, samples, make, oracle, PARAMS)
        assert out["found"] and out["n_good"] >= 100 and not took_widening_search(out["trace"]), rig_kind
        assert max(ref.pose_error(out["Tcw"][:3, :3], out["Tcw"][:3, 3], truth["R"], truth["t"])) < 0.02
        frame, rig, cands, truth, samples = chain_case("none", rig_kind)
        out = rref.relocalize(frame, rig, cands, samples, make, oracle, PARAMS)
        assert not out["found"] and (out["mp_ref"] == -1).all() and not out["outlier"].any()
        last = {v["cand"]: v for v in out["trace"]}
        assert len(last) == 3 and all(v["no_more"] for v in last.values()) and not any(v["found"] for v in out["trace"])
        # 120 true matches 1.5-12 m away: what the chain makes of the parallax in usun (a report; the GPU test asks for parity)
        frame, rig, cands, truth, samples = chain_case("deep", rig_kind)
        out = rref.relocalize(frame, rig, cands, samples, make, oracle, PARAMS)
        print("%s, map points 1.5-12 m away: found %s, n_good %d, visits %s" % (
            rig_kind, out["found"], out["n_good"], [(v["call"], v["found"], v["no_more"], v["n_inliers"]) for v in out["trace"]]))
        assert out["trace"][0]["n_inliers"] >= 100 and len(out["trace"]) >= 2  # the PnP stage ran on the BoW matches


def test_rig_records_match_the_header(tmp_path):
    """sizeof / offsetof of vieo_pnp_rig and vieo_reloc_rig as gcc sees include/vieo_hot.h against the numpy dtypes"""
    prog = r"""
#include <stdio.h>
#include <stddef.h>
#include "vieo_hot.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  printf("vieo_camera %zu\n", sizeof(vieo_camera));
  printf("vieo_pnp_rig %zu\n", sizeof(vieo_pnp_rig));
  F(vieo_pnp_rig, n_cams); F(vieo_pnp_rig, reserved); F(vieo_pnp_rig, cams); F(vieo_pnp_rig, Tcr); F(vieo_pnp_rig, Trc);
  printf("vieo_reloc_rig %zu\n", sizeof(vieo_reloc_rig));
  F(vieo_reloc_rig, pnp); F(vieo_reloc_rig, cam_first); F(vieo_reloc_rig, sbp); F(vieo_reloc_rig, pose_cams);
  return 0;
}
"""
    from vieo_slam_amd.ba_types import CAMERA_DTYPE
    src = tmp_path / "sizes.c"
    src.write_text(prog)
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in subprocess.check_output([exe]).decode().strip().splitlines())}
    assert (got["vieo_camera"], got["vieo_pnp_rig"], got["vieo_reloc_rig"]) == (152, 1384, 1408)
    assert CAMERA_DTYPE.itemsize == got["vieo_camera"]
    for name, dt in (("vieo_pnp_rig", rl.PNP_RIG_DTYPE), ("vieo_reloc_rig", rl.RELOC_RIG_DTYPE)):
        assert got[name] == dt.itemsize, name
        for f in dt.names:
            assert got["%s.%s" % (name, f)] == dt.fields[f][1], (name, f)
