"""GPU parity: HIP Hamming matching (knn-2, rectified stereo) vs the CPU oracle, bit-exact.

knn-2 has two kernels: k_knn2_mfma (the default) and the popcount kernel k_knn2, chosen by VIEO_KNN2_MFMA=0, which is
read once per process: test_knn2_popcount_kernel runs every knn-2 case of this file in a fresh child process with it
set and compares the child's bytes with this process's and with the oracle.  vieo_hamming_knn2_batch_device (a table
of jobs over one descriptor block, rows [num_mono, n) of each camera) is called by test_knn2_batch_device."""
import os
import subprocess
import sys

import numpy as np
import pytest

from vieo_slam_amd import synth
from vieo_slam_amd._lib import DeviceBuffer, check, lib

pytestmark = pytest.mark.gpu
BF, BASELINE = synth.EUROC_BF, synth.EUROC_BF / synth.EUROC_FX


def _hip(nfeat=1200):
    from vieo_slam_amd.orb_extractor import ORBextractor
    return ORBextractor(nfeat, 1.2, 8, 20, 7)


KNN2_SHAPES = [(1200, 1200), (1500, 1000), (1, 1), (7, 1), (65, 130), (3, 0), (300, 33), (257, 31), (40, 2100)]


def _parity_inputs(nq, nt):
    q = synth.synth_descriptors(nq, seed=7, n_dup=nq // 2)
    t = synth.synth_descriptors(max(nt, 1), seed=8, n_dup=nt // 2)[:nt]
    if nt > 50:
        t[40] = t[10]
        q[0] = t[10]
    return q, t


@pytest.mark.parametrize("nq,nt", KNN2_SHAPES)
def test_knn2_parity(oracle, nq, nt):
    from vieo_slam_amd.matching import knn_match2
    q, t = _parity_inputs(nq, nt)
    oi, od = oracle.knn2(q, t) if nt > 0 else (np.full((nq, 2), -1, np.int32),
                                               np.full((nq, 2), np.iinfo(np.int32).max, np.int32))
    hi, hd = knn_match2(q, t)
    assert np.array_equal(oi, hi) and np.array_equal(od, hd)


def _extreme_inputs():
    rng = np.random.default_rng(5)
    q = rng.integers(0, 256, (70, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (45, 32), dtype=np.uint8)
    q[0], q[1], q[2] = 0, 255, t[7]
    t[0], t[1], t[20], t[21], t[44] = 255, 0, t[7], 0, 255
    return q, t


def test_knn2_extreme_rows(oracle):
    """all-zero / all-one rows (|a| = 0, 256; a.b = 0, 256) and exact duplicates among the train rows: the matrix-core form
    computes |a| + |b| - 2 a.b, its packed keys must order exactly like the distances + indices"""
    from vieo_slam_amd.matching import knn_match2
    q, t = _extreme_inputs()
    oi, od = oracle.knn2(q, t)
    hi, hd = knn_match2(q, t)
    assert np.array_equal(oi, hi) and np.array_equal(od, hd)
    assert od[0, 0] == 0 and oi[0, 0] == 1 and od[1, 0] == 0 and oi[1, 0] == 0 and oi[2].tolist() == [7, 20]


def _real_inputs(oracle):
    left, right, _ = synth.synth_stereo_pair(1001)
    _, _, dl = oracle.extractor(1200)(left)
    _, _, dr = oracle.extractor(1200)(right)
    return dl, dr


def test_knn2_real_descriptors_with_ties(oracle):
    from vieo_slam_amd.matching import knn_match2
    dl, dr = _real_inputs(oracle)
    oi, od = oracle.knn2(dl, dr)
    hi, hd = knn_match2(dl, dr)
    assert np.array_equal(oi, hi) and np.array_equal(od, hd)


# ---- vieo_hamming_knn2_batch_device: camera c holds KNN2_CAMS[c] = (n, num_mono) rows of a block of KNN2_CAP rows a camera;
# a job (q, t) searches rows [num_mono, n) of camera q in those of camera t.  The sizes n - num_mono:
#   255, 256, 257    around the 256 queries of a k_knn2_mfma workgroup (and four 64-query workgroups of k_knn2)
#   31 .. 33, 63 .. 65  around its tiles of 32 train rows;  0 and 1: no train row, no second neighbour
KNN2_CAP = 400
KNN2_CAMS = [(300, 45), (263, 7), (357, 100), (34, 3), (32, 0), (38, 5), (64, 1), (66, 2), (74, 9), (12, 12), (6, 5), (400, 0)]
KNN2_JOBS = [(0, 3), (1, 4), (2, 5), (0, 6), (1, 7), (2, 8), (9, 0), (0, 9), (2, 10), (10, 10), (3, 2), (11, 11), (8, 1), (4, 4)]
KNN2_GUARD = -0x21524111


def _batch_inputs():
    desc = np.zeros((len(KNN2_CAMS), KNN2_CAP, 32), np.uint8)
    for c, (n, m) in enumerate(KNN2_CAMS):
        desc[c] = synth.synth_descriptors(KNN2_CAP, seed=60 + c, n_dup=KNN2_CAP // 2)
    desc[3, 3 + 30] = desc[3, 3 + 2]    # equal train rows: in one tile, across two tiles, the last row of a job
    desc[8, 9 + 64] = desc[8, 9 + 31]
    desc[6, 1 + 62] = desc[6, 1 + 0]
    desc[0, 45 + 254] = desc[3, 3 + 2]  # the last query of a job meets them at distance 0
    desc[2, 100 + 256] = desc[8, 9 + 31]
    return desc


def _knn2_batch(desc):
    """(idx, dist) [n_jobs, KNN2_CAP, 2] of one vieo_hamming_knn2_batch_device call, guard pattern where nothing is written"""
    counts = np.array(KNN2_CAMS, np.int32)
    pairs = np.array(KNN2_JOBS, np.int32)
    nj = len(pairs)
    d_desc, d_idx, d_dist = DeviceBuffer(desc.nbytes), DeviceBuffer(nj * KNN2_CAP * 8), DeviceBuffer(nj * KNN2_CAP * 8)
    d_desc.upload(desc)
    guard = np.full((nj, KNN2_CAP, 2), KNN2_GUARD, np.int32)
    d_idx.upload(guard), d_dist.upload(guard)
    check(lib().vieo_hamming_knn2_batch_device(d_desc.ptr, counts.ctypes.data, KNN2_CAP, pairs.ctypes.data, nj, d_idx.ptr,
                                               d_dist.ptr, None), "vieo_hamming_knn2_batch_device")
    check(lib().vieo_device_synchronize(), "sync")
    out = d_idx.download(np.int32, (nj, KNN2_CAP, 2)), d_dist.download(np.int32, (nj, KNN2_CAP, 2))
    for b in (d_desc, d_idx, d_dist):
        b.free()
    return out


def _assert_knn2_batch(oracle, desc, idx, dist):
    sizes = set()
    for j, (qc, tc) in enumerate(KNN2_JOBS):
        (nq_all, qm), (nt_all, tm) = KNN2_CAMS[qc], KNN2_CAMS[tc]
        q, t = desc[qc, qm:nq_all], desc[tc, tm:nt_all]
        sizes.add((len(q), len(t)))
        if len(t) and len(q):
            oi, od = oracle.knn2(q, t)
        else:
            oi, od = np.full((len(q), 2), -1, np.int32), np.full((len(q), 2), np.iinfo(np.int32).max, np.int32)
        assert np.array_equal(idx[j, :len(q)], oi) and np.array_equal(dist[j, :len(q)], od), (j, qc, tc)
        assert (idx[j, len(q):] == KNN2_GUARD).all() and (dist[j, len(q):] == KNN2_GUARD).all(), (j, "rows no job owns were written")
    assert {a for a, _ in sizes} >= {0, 1, 255, 256, 257} and {b for _, b in sizes} >= {0, 1, 31, 32, 33, 63, 64, 65}


def test_knn2_batch_device(oracle):
    desc = _batch_inputs()
    idx, dist = _knn2_batch(desc)
    _assert_knn2_batch(oracle, desc, idx, dist)
    assert idx[0, 254].tolist() == [2, 30] and dist[0, 254].tolist()[0] == 0  # the planted tie: the lower train row first


def _all_knn2_outputs(oracle):
    """every knn-2 case of this file on the device, as a dict of arrays"""
    from vieo_slam_amd.matching import knn_match2
    cases = [_parity_inputs(nq, nt) for nq, nt in KNN2_SHAPES] + [_extreme_inputs(), _real_inputs(oracle)]
    out = {}
    for k, (q, t) in enumerate(cases):
        out["idx%d" % k], out["dist%d" % k] = knn_match2(q, t)
    out["batch_idx"], out["batch_dist"] = _knn2_batch(_batch_inputs())
    return cases, out


POPCOUNT_CHILD = """
import sys
import numpy as np
sys.path.insert(0, %r)
from tests import oracle_lib, test_matching_parity as t
np.savez(sys.argv[1], **t._all_knn2_outputs(oracle_lib.load())[1])
"""


def test_knn2_popcount_kernel(oracle, tmp_path):
    """k_knn2 (VIEO_KNN2_MFMA=0, read once per process: a fresh child) on every knn-2 case of this file: the same bytes as
    the matrix-core kernel of this process, and the oracle's"""
    assert os.environ.get("VIEO_KNN2_MFMA", "1") != "0", "this process must run the default kernel"
    cases, here = _all_knn2_outputs(oracle)
    script = tmp_path / "popcount.py"
    script.write_text(POPCOUNT_CHILD % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    r = subprocess.run([sys.executable, str(script), str(tmp_path / "popcount.npz")], env=dict(os.environ, VIEO_KNN2_MFMA="0"),
                       timeout=120, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    child = np.load(tmp_path / "popcount.npz")
    assert sorted(child.files) == sorted(here)
    for k in here:
        assert np.array_equal(here[k].view(np.uint8), np.ascontiguousarray(child[k]).view(np.uint8)), k
    for k, (q, t) in enumerate(cases):
        if len(t):
            oi, od = oracle.knn2(q, t)
            assert np.array_equal(child["idx%d" % k], oi) and np.array_equal(child["dist%d" % k], od), k
    _assert_knn2_batch(oracle, _batch_inputs(), child["batch_idx"], child["batch_dist"])


@pytest.mark.parametrize("seed", [1000, 1001, 1002])
def test_stereo_rectified_host_api(oracle, seed):
    from vieo_slam_amd.matching import compute_stereo_matches
    left, right, _ = synth.synth_stereo_pair(seed)
    oL, oR = oracle.extractor(1200), oracle.extractor(1200)
    _, kl, dl = oL(left)
    _, kr, dr = oR(right)
    our, odp = oracle.stereo_match(oL, oR, kl, dl, kr, dr, BASELINE, BF)
    hL, hR = _hip(), _hip()
    _, hkl, hdl = hL(left)
    _, hkr, hdr = hR(right)
    assert np.array_equal(hkl, kl) and np.array_equal(hdr, dr)
    hur, hdp = compute_stereo_matches(hL, hR, hkl, hdl, hkr, hdr, BASELINE, BF)
    assert (our >= 0).sum() > 300
    assert np.array_equal(our.view(np.uint32), hur.view(np.uint32))
    assert np.array_equal(odp.view(np.uint32), hdp.view(np.uint32))


def test_stereo_rectified_edge_cases(oracle):
    from vieo_slam_amd.matching import compute_stereo_matches
    left, right, _ = synth.synth_stereo_pair(1003)
    oL, oR = oracle.extractor(1200), oracle.extractor(1200)
    _, kl, dl = oL(left)
    _, kr, dr = oR(right)
    hL, hR = _hip(), _hip()
    hL(left), hR(right)
    # no right keys at all; a handful of right keys; unrelated right image (few/no matches)
    for sel in (slice(0, 0), slice(0, 5)):
        our, odp = oracle.stereo_match(oL, oR, kl, dl, kr[sel], dr[sel], BASELINE, BF)
        hur, hdp = compute_stereo_matches(hL, hR, kl, dl, kr[sel], dr[sel], BASELINE, BF)
        assert np.array_equal(our.view(np.uint32), hur.view(np.uint32))
        assert np.array_equal(odp.view(np.uint32), hdp.view(np.uint32))
    other = synth.synth_image(2000)
    _, k2, d2 = oR(other)
    hR(other)
    our, odp = oracle.stereo_match(oL, oR, kl, dl, k2, d2, BASELINE, BF)
    hur, hdp = compute_stereo_matches(hL, hR, kl, dl, k2, d2, BASELINE, BF)
    assert np.array_equal(our.view(np.uint32), hur.view(np.uint32))
    assert np.array_equal(odp.view(np.uint32), hdp.view(np.uint32))


def test_stereo_rectified_batch_device(oracle):
    from vieo_slam_amd.orb_extractor import KEYPOINT_DTYPE
    F = 4
    imgs = np.zeros((F, 2, 480, 752), np.uint8)
    for f in range(F):
        imgs[f, 0], imgs[f, 1], _ = synth.synth_stereo_pair(1040 + f)
    h = _hip()
    cap = h.max_keypoints()
    d_img = DeviceBuffer(imgs.nbytes)
    d_img.upload(imgs)
    n_img = 2 * F
    d_kp, d_desc, d_cnt = DeviceBuffer(n_img * cap * 28), DeviceBuffer(n_img * cap * 32), DeviceBuffer(n_img * 8)
    d_ur, d_dp = DeviceBuffer(F * cap * 4), DeviceBuffer(F * cap * 4)
    h.extract_batch_device(d_img.ptr, n_img, 752, 480, 752, 752 * 480, d_kp.ptr, d_desc.ptr, cap, d_cnt.ptr)
    check(lib().vieo_stereo_match_rectified_batch_device(h._h, F, d_kp.ptr, d_desc.ptr, d_cnt.ptr, cap,
                                                         BASELINE, BF, d_ur.ptr, d_dp.ptr))
    h.sync()
    cnt = d_cnt.download(np.int32, (n_img, 2))
    ur = d_ur.download(np.float32, (F, cap))
    dp = d_dp.download(np.float32, (F, cap))
    oL, oR = oracle.extractor(1200), oracle.extractor(1200)
    for f in range(F):
        _, kl, dl = oL(imgs[f, 0])
        _, kr, dr = oR(imgs[f, 1])
        our, odp = oracle.stereo_match(oL, oR, kl, dl, kr, dr, BASELINE, BF)
        n = cnt[2 * f, 0]
        assert n == len(kl)
        assert np.array_equal(our.view(np.uint32), ur[f, :n].view(np.uint32)), f
        assert np.array_equal(odp.view(np.uint32), dp[f, :n].view(np.uint32)), f
