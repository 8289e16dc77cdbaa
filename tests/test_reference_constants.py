"""Build-container check: data tables and named constants parsed straight out of the
reference's sources and compared with what the oracle and the HIP product carry.  /root/reference does not exist on
the GPU box, so every test here skips without it (and none is marked gpu)."""
import os
import re

import numpy as np
import pytest

REF = os.environ.get("VIEO_REFERENCE_ROOT", "/root/reference")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src")), reason="no reference checkout here")


def _read(*parts):
    with open(os.path.join(*parts), errors="replace") as f:
        return f.read()


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


# the bundle-adjustment engine's translation unit: lba.hip and the stage headers it is cut into
LBA_SOURCES = ("lba.hip", "lba_device.h", "lba_inertial_device.h", "lba_state_device.h", "lba_linearize_device.h",
               "lba_schur_device.h", "lba_solve_device.h")


def _read_lba():
    return "".join(_read(ROOT, "vieo_slam_amd", "csrc", f) for f in LBA_SOURCES)


def _const(text, name):
    m = re.search(r"\b%s\s*=\s*([-+0-9.eE]+)f?\s*[;,]" % re.escape(name), text)
    assert m, name
    return float(m.group(1))


def test_brief_pattern_equals_reference_table():
    """bit_pattern_31_[256 * 4] (src/ORBextractor.cc:129-389) == include/vieo_orb_pattern_31.h, all 1024 ints."""
    src = _strip_comments(_read(REF, "src", "ORBextractor.cc"))
    m = re.search(r"bit_pattern_31_\s*\[\s*256\s*\*\s*4\s*\]\s*=\s*\{(.*?)\}\s*;", src, flags=re.S)
    assert m
    ref = np.array([int(t) for t in re.findall(r"-?\d+", m.group(1))])
    hdr = _strip_comments(_read(ROOT, "include", "vieo_orb_pattern_31.h"))
    m2 = re.search(r"VIEO_ORB_PATTERN_31\s*\[\s*256\s*\*\s*4\s*\]\s*=\s*\{(.*?)\}\s*;", hdr, flags=re.S)
    assert m2
    ours = np.array([int(t) for t in re.findall(r"-?\d+", m2.group(1))])
    assert ref.shape == ours.shape == (1024,)
    assert np.array_equal(ref, ours)
    assert np.abs(ref).max() <= 13  # fits the 31 x 31 patch after rotation (radius 19 = EDGE_THRESHOLD)


def test_extractor_constants():
    src = _strip_comments(_read(REF, "src", "ORBextractor.cc"))
    ours = _strip_comments(_read(ROOT, "oracle", "orb_extractor.cc"))
    for name in ("PATCH_SIZE", "HALF_PATCH_SIZE", "EDGE_THRESHOLD"):
        assert _const(src, name) == _const(ours, name), name
    # FAST cell size (ORBextractor.cc:726): const float W = 35 in the reference, the oracle and the product's planner
    assert _const(src, "W") == 35 == _const(ours, "W")
    assert _const(_strip_comments(_read(ROOT, "vieo_slam_amd", "csrc", "orb_extractor.hip")), "W") == 35


def test_matcher_constants():
    src = _strip_comments(_read(REF, "src", "ORBmatcher.cc"))
    ref = {n: _const(src, "ORBmatcher::" + n) for n in ("TH_HIGH", "TH_LOW", "HISTO_LENGTH")}
    assert ref == {"TH_HIGH": 100, "TH_LOW": 50, "HISTO_LENGTH": 30}
    t = _strip_comments(_read(ROOT, "oracle", "matching.cc"))
    assert _const(t, "TH_HIGH") == ref["TH_HIGH"] and _const(t, "TH_LOW") == ref["TH_LOW"]
    t = _strip_comments(_read(ROOT, "vieo_slam_amd", "csrc", "orb_match.h"))  # the one place the kernels take them from
    assert _const(t, "kThHigh") == ref["TH_HIGH"] and _const(t, "kThLow") == ref["TH_LOW"]
    assert _const(t, "kHistoLen") == ref["HISTO_LENGTH"]
    t = _strip_comments(_read(ROOT, "oracle", "proj_search.cc"))
    assert _const(t, "TH_HIGH_") == ref["TH_HIGH"] and _const(t, "HISTO_LENGTH") == ref["HISTO_LENGTH"]
    from vieo_slam_amd import matching
    text = _read(ROOT, "vieo_slam_amd", "matching.py")
    assert "TH_LOW, TH_HIGH, HISTO_LENGTH = 50, 100, 30" in text and matching is not None


def test_optimizer_thresholds_are_the_reference_literals():
    """chi2 gates and Huber widths appear as these literals in the reference and in both restatements."""
    opt_h = _strip_comments(_read(REF, "include", "Optimizer.h"))
    opt_cc = _strip_comments(_read(REF, "src", "Optimizer.cc"))
    for lit in ("5.991", "7.815", "16.919", "12.592"):
        assert lit in opt_h or lit in opt_cc, lit
    assert "sqrt(5.99)" in opt_cc and "sqrt(7.815)" in opt_cc  # thHuber2D / thHuber3D of the full BAs (:1063-1064)
    ours = _read_lba() + "".join(_read(ROOT, *p) for p in (("oracle", "local_ba_vio.cc"), ("oracle", "pose_opt_vio.cc"),
                                                           ("vieo_slam_amd", "csrc", "pose_opt_vio.hip")))
    for lit in ("5.991", "7.815", "16.919", "12.592", "5.99"):
        assert lit in ours, lit
    # inertial information x 1e-2 behind a fixed state (Optimizer.cc:254,297) and the bias walk's dt fallback of 15
    assert "1e-2" in opt_cc and "deltatij = 15" in opt_cc
    assert "deltatij = 15" in _read(ROOT, "oracle", "local_ba_vio.cc")
    assert "deltatij = 15" in _read_lba()


def test_lm_constants_of_g2o():
    lm = _strip_comments(_read(REF, "optimizer", "g2o", "g2o", "core", "optimization_algorithm_levenberg.cpp"))
    # tau = 1e-5, at most 10 lambda trials, lambda factors 1/3 .. 2/3
    assert re.search(r"_tau\s*=\s*1e-5", lm) and re.search(r'"maxTrialsAfterFailure",\s*10\)', lm)
    assert re.search(r"_goodStepUpperScale\s*=\s*2\.\s*/\s*3\.", lm) and re.search(r"_goodStepLowerScale\s*=\s*1\.\s*/\s*3\.", lm)
    ours = _read_lba()  # the device computes the initial lambda ...
    policy = _read(ROOT, "vieo_slam_amd", "csrc", "lba_policy.h")  # ... the host runs the trials' policy
    assert "1e-5 * s_m[0]" in ours and "H.qmax < 10" in policy and "2. / 3." in policy and "1. / 3." in policy


def test_full_ba_of_the_reference_runs_with_the_scale_vertex():
    """System::FinalGBA passes bScaleOpt = true (src/System.cc:24-33): the form tests/test_global_ba_scale.py covers."""
    sysc = _strip_comments(_read(REF, "src", "System.cc"))
    m = re.search(r"void System::FinalGBA.*?\n}\n", sysc, flags=re.S)
    assert m and re.search(r"GlobalBundleAdjustmentNavStatePRV\([^;]*bRobust,\s*true\)", m.group(0), flags=re.S)
    g = _strip_comments(_read(REF, "src", "Odom", "g2otypes.h"))
    assert re.search(r"typedef EdgeReproject<2, 6, 3, 1> EdgeReprojectPRS;", g)
    assert re.search(r"typedef EdgeReproject<3, 6, 3, 1> EdgeReprojectPRSStereo;", g)


def test_pinning_recipe_configures_or_says_why_not(tmp_path):
    """oracle/ref_build/ (tools/rebaseline_with_reference.sh): with OpenCV >= 4.5 present the reference's own
    ORBextractor.cc is configured for a build into oracle/_ref/; without it the recipe stops with the reason."""
    import shutil
    import subprocess
    if shutil.which("cmake") is None:
        pytest.skip("no cmake")
    r = subprocess.run(["cmake", "-S", os.path.join(ROOT, "oracle", "ref_build"), "-B", str(tmp_path),
                        "-DVIEO_REFERENCE_ROOT=" + REF], capture_output=True, text=True, timeout=120)
    if r.returncode != 0:
        assert "OpenCV >= 4.5 not found" in r.stderr, r.stderr[-2000:]
    else:
        assert os.path.exists(os.path.join(str(tmp_path), "Makefile")) or os.path.exists(
            os.path.join(str(tmp_path), "build.ninja"))
