"""The C++ side of the drop-in boundary: shim/ORBmatcher_hot.cc, shim/Optimizer_hot.cc and
include/vieo_shim.hpp are type-checked with `g++ -fsyntax-only` against declaration-only stand-ins of the reference's
headers and of OpenCV / Eigen / Sophus (tests/shim_compile/mock: none of those libraries exist in the image).  This
is a syntax and ABI check, not parity evidence.  examples/cabi_demo.cc links libvieo_hot.so and drives the C-ABI
without Python; on a GPU box it must run to completion.  shim/OdomPreIntegrator_hot.cc is also linked and run
(tests/shim_compile/preint_driver.cc) and its members are compared with the oracle's."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "shim_compile", "mock")
INC = ["-I" + MOCK, "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "shim")]


@pytest.mark.parametrize("src", ["shim/ORBmatcher_hot.cc", "shim/Optimizer_hot.cc", "shim/Frame_hot.cc", "shim/Tracking_hot.cc",
                                 "shim/OdomPreIntegrator_hot.cc", "tests/shim_compile/use_extractor_shim.cc"])
def test_shim_translation_unit_type_checks(src):
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror"] + INC + [os.path.join(ROOT, src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_shims_define_every_replaced_member():
    """the definitions the reference tree loses are all present in the shim sources"""
    m = open(os.path.join(ROOT, "shim", "ORBmatcher_hot.cc")).read()
    for sig in ("int ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame",
                "int ORBmatcher::SearchByProjection(Frame& F, const vector<MapPoint*>& vpMapPoints",
                "int ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF",
                "int ORBmatcher::SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2",
                "void ORBmatcher::SearchByProjectionBase(", "int ORBmatcher::Fuse(KeyFrame* pKF, const vector<MapPoint*>&"):
        assert sig in m, sig
    o = open(os.path.join(ROOT, "shim", "Optimizer_hot.cc")).read()
    for sig in ("int Optimizer::PoseOptimization(Frame* pFrame, Frame* pLastF)",
                "int Optimizer::PoseOptimization<Frame>(", "int Optimizer::PoseOptimization<KeyFrame>(",
                "void Optimizer::LocalBundleAdjustmentNavStatePRV(KeyFrame* pKF, int Nlocal, bool* pbStopFlag, Map* pMap",
                "void Optimizer::LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Map* pMap, int Nlocal)",
                "MapPoint::mGlobalMutex", "pMap->mMutexMapUpdate", "pbStopFlag",
                # round 6: the full BAs and the batched UpdateNormalAndDepth of every write-back (8f-3)
                "int Optimizer::GlobalBundleAdjustmentNavStatePRV(Map* pMap, const cv::Mat& cvgw, int nIterations, bool* pbStopFlag",
                "void Optimizer::BundleAdjustment(const std::vector<KeyFrame*>& vpKFs, const std::vector<MapPoint*>& vpMP, int nIterations",
                "void Optimizer::GlobalBundleAdjustment(Map* pMap, int nIterations, bool* pbStopFlag",
                "vieo_global_bundle_adjustment_vio_scale", "vieo_bundle_adjustment_enc", "vieo_update_normal_and_depth_batch"):
        assert sig in o, sig
    assert "->UpdateNormalAndDepth()" not in o  # (no per-point host call is left in a write-back)
    f = open(os.path.join(ROOT, "shim", "Frame_hot.cc")).read()
    for sig in ("void Frame::ComputeStereoMatches()", "void Frame::ComputeStereoFishEyeMatches(const float th_far_pts)",
                "vieo_stereo_match_rectified_resident", "vieo_stereo_fisheye_match", "vieo_orb_holds"):
        assert sig in f, sig
    t = open(os.path.join(ROOT, "shim", "Tracking_hot.cc")).read()
    for sig in ("bool Tracking::TrackWithIMU(bool bMapUpdated)", "bool Tracking::TrackLocalMapWithIMU(bool bMapUpdated)",
                "bool Tracking::TrackWithMotionModel()", "bool Tracking::TrackLocalMap()", "vieo_track_frame",
                "vieo_tracker_create_rig", "P.vision_only",
                "void Tracking::SearchLocalPoints()", "vieo_is_in_frustum_batch", "IncreaseVisible", "GetLastChangeIdx", "ensure_mode"):
        assert sig in t, sig
    pi = open(os.path.join(ROOT, "shim", "OdomPreIntegrator_hot.cc")).read()
    for sig in ("int IMUPreIntegratorBase<IMUDataBase>::PreIntegration(const double& timeStampi, const double& timeStampj",
                "vieo_imu_preintegrate_batch", "VIEO_PREINT_GAP"):
        assert sig in pi, sig
    # the resident frame is what the matcher shim tries first
    for sig in ("vieo_search_by_projection_last_frame_resident", "vieo_search_by_projection_resident", "vieo_orb_holds"):
        assert sig in m, sig


def _build_demo():
    exe = os.path.join(ROOT, "examples", "cabi_demo")
    lib = os.path.join(ROOT, "vieo_slam_amd")
    assert os.path.exists(os.path.join(lib, "libvieo_hot.so")), "build libvieo_hot.so first (__graft_entry__.build())"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "cabi_demo.cc"), "-o", exe, "-L" + lib, "-lvieo_hot",
                           "-Wl,-rpath,$ORIGIN/../vieo_slam_amd"])
    return exe


def test_cabi_demo_links_without_python():
    exe = _build_demo()
    r = subprocess.run([exe], capture_output=True, text=True)
    # 0 on a GPU box; 2 = "no gfx950 device" (the loud no-fallback exit) where there is none
    assert r.returncode in (0, 2), (r.returncode, r.stdout, r.stderr)
    if r.returncode == 2:
        assert "no CPU fallback" in r.stderr


@pytest.mark.gpu
def test_cabi_demo_runs_on_gpu():
    exe = os.path.join(ROOT, "examples", "cabi_demo")
    if not os.path.exists(exe):
        exe = _build_demo()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "cabi_demo ok" in r.stdout and "vieo_pose_optimization_vio" in r.stdout


# ---------------------------------------------------------------- the pre-integration shim, executed -----------
# tests/shim_compile/preint_driver.cc links shim/OdomPreIntegrator_hot.cc (against the mock headers, whose Eigen::Matrix
# is a working value type) with libvieo_hot.so and runs IMUPreIntegratorBase<IMUDataBase>::PreIntegration the way
# Tracking::PreIntegration does: breset = true from the key frame, then breset = false continuations.

def _build_preint_driver(out_dir):
    lib = os.path.join(ROOT, "vieo_slam_amd")
    assert os.path.exists(os.path.join(lib, "libvieo_hot.so")), "build libvieo_hot.so first (__graft_entry__.build())"
    exe = os.path.join(str(out_dir), "preint_driver")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + INC +
                       [os.path.join(ROOT, "tests", "shim_compile", "preint_driver.cc"),
                        os.path.join(ROOT, "shim", "OdomPreIntegrator_hot.cc"), "-o", exe, "-L" + lib, "-lvieo_hot",
                        "-Wl,-rpath," + lib], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _preint_scenario(fixed):
    """one IMU list with a 2 s hole; a key frame between two samples; frame times on samples and between them; one
    continuation with no samples; the last one across the hole.  returns (noise, samples, calls) with calls
    [(ti, tj, i0, i1, breset, bg, ba)]"""
    import numpy as np
    from tests.test_imu_preint import _noise, _samples
    rng = np.random.default_rng(31)
    s = _samples(rng, 40.0, 160, jitter=0.001)
    s["t"][130:] += 2.0
    t = s["t"]
    times = [t[5] + 0.0017, t[12], t[19] + 0.0011, t[27], t[27], t[40], t[55] + 0.0023, t[70], t[90], t[128],
             t[140] + 0.0012]
    bg, ba = rng.normal(0, 0.01, 3), rng.normal(0, 0.05, 3)
    calls = []
    for k in range(1, len(times)):
        t0, t1 = times[k - 1], times[k]
        i0 = max(int(np.searchsorted(t, t0, "right")) - 1, 0)   # iteri: the last sample at or before t0
        i1 = min(int(np.searchsorted(t, t1, "left")) + 1, len(s))  # ++iterj: one past the first at or after t1
        if t0 == t1:
            i1 = i0  # (a frame with nothing to integrate)
        calls.append((t0, t1, i0, i1, 1 if k == 1 else 0, bg, ba))
    return _noise(fixed), s, calls


def _write_preint_input(path, noise, s, calls):
    import numpy as np
    v = [len(s)]
    for x in s:
        v += [x["t"]] + list(x["w"]) + list(x["a"])
    v += list(noise[0]["sigma_g"]) + list(noise[0]["sigma_a"]) + [noise[0]["freq_ref"], noise[0]["dt_cov_noise_fixed"]]
    v.append(len(calls))
    for ti, tj, i0, i1, breset, bg, ba in calls:
        v += [ti, tj, i0, i1, breset] + list(bg) + list(ba)
    np.asarray(v, np.float64).tofile(path)


def test_preint_driver_builds_and_links(tmp_path):
    exe = _build_preint_driver(tmp_path)
    _write_preint_input(str(tmp_path / "in.bin"), *_preint_scenario(1))
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                       timeout=300)
    # 0 on a GPU box; 2 = "no gfx950 device" (the loud no-fallback exit) where there is none
    assert r.returncode in (0, 2), (r.returncode, r.stdout, r.stderr)
    if r.returncode == 2:
        assert "no CPU fallback" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("fixed", [1, 0])
def test_preint_shim_continuations_match_oracle(tmp_path, oracle, fixed):
    """the shim's members after every call against the oracle's chained calls (seeded with its previous output), to
    the tolerances of test_imu_preint.py::test_preintegration_parity; return values 0 / -1 as the reference's"""
    import numpy as np
    from vieo_slam_amd.ba_types import IMU_PREINT_DTYPE
    exe = _build_preint_driver(tmp_path)
    noise, s, calls = _preint_scenario(fixed)
    _write_preint_input(str(tmp_path / "in.bin"), noise, s, calls)
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    got = np.fromfile(str(tmp_path / "out.bin"), np.float64).reshape(len(calls), 224)
    seed, seed_prv = np.zeros(1, IMU_PREINT_DTYPE), np.zeros((1, 9, 9))
    statuses = []
    for c, (ti, tj, i0, i1, breset, bg, ba) in enumerate(calls):
        o, p, st = oracle.imu_preintegrate(noise, [s[i0:i1]], [ti], [tj], [bg], [ba], seed, seed_prv, [breset])
        seed, seed_prv = o, p
        statuses.append(int(st[0]))
        g = got[c]
        assert g[0] == (-1 if st[0] == 2 else 0), (c, g[0], st[0])
        members = np.concatenate([o[0][k].reshape(-1) for k in ("dt", "Rij", "vij", "pij", "JgR", "Jgv", "Jav", "Jgp",
                                                                  "Jap")])
        assert np.allclose(g[1:62], members, rtol=1e-11, atol=1e-13), c
        for a, b in ((o[0]["Sigma"], g[62:143]), (p.reshape(81), g[143:224])):
            assert np.array_equal(np.isnan(a), np.isnan(b)), c
            a, b = np.nan_to_num(a), np.nan_to_num(b)
            assert np.abs(a - b).max() / (np.abs(a).max() + 1e-300) < 1e-10, c
    # the scenario covers a reset, plain continuations, an empty one and a gap
    assert statuses[0] == 0 and 1 in statuses and statuses[-1] == 2 and got[-1][1] == 0
