"""The host half of the feature-vector searches (vieo_slam_amd/csrc/bow_walk.h over orb_match.h): the query plan and the
order-dependent walk of both SearchByBoW forms, the rotation bin, ComputeThreeMaxima as a mask, the node-table check
and the shared-node enumeration, against the Python restatements the GPU tests use (reloc_ref.search_by_bow,
reloc_rig_ref.search_by_bow, loop_ref.search_by_bow_kf, reloc_ref.three_maxima).  CPU only: the headers are compiled
with g++ (tests/emul/bow_walk_emul.cc), which fills the distance array with the header's own host Hamming function in
the place of k_bow_distances; the device fills it in test_relocalization*.py and test_loop_sim3.py.

The rotation bin is round(rot / HISTO_LENGTH) as in the reference (factor = 1 / HISTO_LENGTH), so angles in [0, 360)
give bins 0 ... 12 and 345 gives 12; `bin == HISTO_LENGTH -> 0` is reached by differences of 885 ... 915 only, which
the function (it does not range-check) is also given here."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from tests import loop_ref, reloc_ref, reloc_rig_ref
from vieo_slam_amd import loop_closing as lc
from vieo_slam_amd import relocalization as rl

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
VIEO_OK, VIEO_E_INVALID = 0, -1
f32 = np.float32
ALL_BINS = (1 << reloc_ref.HISTO_LENGTH) - 1


@functools.lru_cache(maxsize=None)
def lib():
    out = os.path.join(HERE, "emul", "libbow_walk_emul.so")
    csrc = os.path.join(ROOT, "vieo_slam_amd", "csrc")
    deps = [os.path.join(HERE, "emul", "bow_walk_emul.cc"), os.path.join(csrc, "bow_walk.h"), os.path.join(csrc, "orb_match.h"),
            os.path.join(ROOT, "include", "vieo_hot.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-o", out, deps[0]])
    L = ctypes.CDLL(out)
    L.bw_error.restype = ctypes.c_char_p
    L.bw_rot_bin.argtypes = [ctypes.c_float, ctypes.c_float]
    L.bw_three_maxima.restype = ctypes.c_uint32
    L.bw_three_maxima.argtypes = [ctypes.c_void_p]
    L.bw_hamming.argtypes = [ctypes.c_void_p] * 2
    L.bw_node_table_ok.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 3
    L.bw_shared_nodes.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    L.bw_search_frame.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_float, ctypes.c_int] + [ctypes.c_void_p] * 2
    L.bw_search_kf.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int, ctypes.c_float, ctypes.c_int] + [ctypes.c_void_p] * 2
    return L


def p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None


def search_frame(kfs, frame, key_cam, nn_ratio, check):
    """all key frames in one call, as vieo_search_by_bow / vieo_search_by_bow_rig take them"""
    recs = np.concatenate([k.rec for k in kfs])
    match = np.full((len(kfs), len(frame.keys)), 7, np.int32)
    n = np.zeros(len(kfs), np.int32)
    rc = lib().bw_search_frame(p(frame.rec), p(key_cam), p(recs), len(kfs), nn_ratio, int(check), p(match), p(n))
    return rc, match, n


def search_kf(kf1, cands, nn_ratio, check):
    recs = np.concatenate([k.rec for k in cands])
    match = np.full((len(cands), len(kf1.keys)), 7, np.int32)
    n = np.zeros(len(cands), np.int32)
    rc = lib().bw_search_kf(p(kf1.rec), p(recs), len(cands), nn_ratio, int(check), p(match), p(n))
    return rc, match, n


def test_constants_and_host_hamming():
    assert [lib().bw_constants(i) for i in range(3)] == [reloc_ref.TH_LOW, 100, reloc_ref.HISTO_LENGTH]
    rng = np.random.default_rng(2)
    d = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    d[1], d[2] = 0, 255
    for i in range(len(d)):
        for j in (0, 1, 2, (i * 7 + 3) % len(d), i):
            assert lib().bw_hamming(p(d[i]), p(d[j])) == reloc_ref.descriptor_distance(d[i], d[j])


# ---------------------------------------------------------------------------------------------------------------------
# SearchByBoW(KeyFrame*, Frame&)
def test_frame_walk_rectified_against_the_restatement():
    frame, kfs = rl.make_bow_scene(1)
    assert len(kfs) == 3 and len(frame.keys) == 300
    total = dict(skipped=0, ratio=0, replaced=0, kept=0, rotation=0)
    for check in (True, False):
        rc, match, n = search_frame(kfs, frame, None, 0.75, check)
        assert rc == VIEO_OK
        for i, kf in enumerate(kfs):
            m, nm, ev = reloc_ref.search_by_bow(kf, frame, 0.75, check)
            assert np.array_equal(match[i], m) and n[i] == nm, (i, check)
            for k in total:
                total[k] += ev[k]
    assert total["skipped"] > 0 and total["ratio"] > 0 and total["replaced"] > 0 and total["rotation"] > 0, total


def test_frame_walk_rig_against_the_restatement():
    frame, key_cam, cam_first, kfs = rl.make_bow_rig_scene(1, 4)
    assert np.diff(cam_first).tolist().count(0) == 1 and len(frame.keys) == 300
    total = dict(skipped=0, ratio=0, replaced=0, kept=0, rotation=0, empty_slot=0, second_image=0)
    zeros = np.zeros_like(key_cam)
    for check in (True, False):
        rc, match, n = search_frame(kfs, frame, key_cam, 0.75, check)
        rc0, match0, n0 = search_frame(kfs, frame, zeros, 0.75, check)  # every key of image 0: the rectified walk
        assert rc == VIEO_OK and rc0 == VIEO_OK
        for i, kf in enumerate(kfs):
            m, nm, ev = reloc_rig_ref.search_by_bow(kf, frame, key_cam, 0.75, check)
            assert np.array_equal(match[i], m) and n[i] == nm, (i, check)
            for k in total:
                total[k] += ev[k]
            r0, rn0, _ = reloc_ref.search_by_bow(kf, frame, 0.75, check)
            assert np.array_equal(match0[i], r0) and n0[i] == rn0 and not np.array_equal(r0, m)
    assert all(total[k] > 0 for k in ("skipped", "ratio", "replaced", "rotation", "empty_slot", "second_image")), total


# ---------------------------------------------------------------------------------------------------------------------
# SearchByBoW(KeyFrame*, KeyFrame*)
def test_kf_walk_against_the_restatement():
    kf1, cands = lc.make_bow_kf_scene(1)
    assert len(cands) == 3 and len(kf1.keys) == 300 and len(kf1.feat_vec) == 40
    total = dict(skipped=0, no_point=0, ratio=0, replaced=0, kept=0, rotation=0)
    for check in (True, False):
        rc, match, n = search_kf(kf1, cands, 0.75, check)
        assert rc == VIEO_OK
        for i, kf2 in enumerate(cands):
            m, nm, ev = loop_ref.search_by_bow_kf(kf1, kf2, 0.75, check)
            assert np.array_equal(match[i], m) and n[i] == nm, (i, check)
            if i == len(cands) - 1:  # no shared node
                assert nm == 0
                continue
            for k in total:
                total[k] += ev[k]
    assert all(v > 0 for v in total.values()), total


def _planted_pair():
    """Two BowKeys of five keys each, two shared nodes, for the rules the generated scenes do not reach.  Right-hand keys
    f0, f1, f2 (node 1) are 160 bits apart; left-hand keys k0, k1, k2 hold ONE map point and lie 30, 20, 25 bits from
    f0, f1, f2: k1 replaces k0's match, the table keeps k0's entry (emplace), so k2 -- worse than k1, better than k0 --
    replaces again.  k3 (another map point) lies 10 bits from f0, which it can take only if the replaced match gave it
    back.  Node 2: k4 lies exactly TH_LOW = 50 bits from g0 and 206 from g1."""
    from vieo_slam_amd.orb_extractor import KEYPOINT_DTYPE
    bits = np.zeros((2, 5, 256), np.uint8)
    for i in range(3):
        bits[1, i, 80 * i:80 * i + 80] = 1   # f0, f1, f2
    bits[1, 4] = 1                           # g1 (g0 = 0)
    for i, clear in enumerate((30, 20, 25)):
        bits[0, i] = bits[1, i]
        bits[0, i, 80 * i:80 * i + clear] = 0   # k0, k1, k2
    bits[0, 3] = bits[1, 0]
    bits[0, 3, 70:80] = 0                    # k3
    bits[0, 4, :50] = 1                      # k4
    desc = np.packbits(bits, axis=2)
    feat_vec = [(1, [0, 1, 2, 3]), (2, [4])], [(1, [0, 1, 2]), (2, [3, 4])]
    left = rl.BowKeys(np.zeros(5, KEYPOINT_DTYPE), desc[0], feat_vec[0], [5, 5, 5, 6, 7])
    right = rl.BowKeys(np.zeros(5, KEYPOINT_DTYPE), desc[1], feat_vec[1], [10, 11, 12, 13, 14])
    return left, right


@pytest.mark.parametrize("check", [True, False])
def test_planted_threshold_and_table_rules(check):
    left, right = _planted_pair()
    # the frame form: TH_LOW itself passes; the table keeps its first entry, so f1 AND f2 end up holding the map point
    m, nm, ev = reloc_ref.search_by_bow(left, right, 0.75, check)
    assert m.tolist() == [3, 1, 2, 4, -1] and nm == 3 and ev["replaced"] == 2
    for key_cam in (None, np.zeros(5, np.uint8)):
        rc, match, n = search_frame([left], right, key_cam, 0.75, check)
        assert rc == VIEO_OK and np.array_equal(match[0], m) and n[0] == nm
    # the key-frame form: TH_LOW itself does not pass; f0 is free again after the replacement
    m, nm, ev = loop_ref.search_by_bow_kf(left, right, 0.75, check)
    assert m.tolist() == [-1, 1, 2, 0, -1] and nm == 2 and ev["replaced"] == 2
    rc, match, n = search_kf(left, [right], 0.75, check)
    assert rc == VIEO_OK and np.array_equal(match[0], m) and n[0] == nm


def test_walks_report_key_angles_outside_the_histogram():
    frame, kfs = rl.make_bow_scene(1)
    angle = kfs[0].keys["angle"].copy()
    try:
        kfs[0].keys["angle"] = 1000.0  # (vieo_search_by_bow refuses this before the walk; the walk keeps its own check)
        rc, _, _ = search_frame(kfs[:1], frame, None, 0.75, True)
        assert rc == VIEO_E_INVALID and lib().bw_error() == b"SearchByBoW: key angles outside [0, 360)"
        assert search_frame(kfs[:1], frame, None, 0.75, False)[0] == VIEO_OK
    finally:
        kfs[0].keys["angle"] = angle
    kf1, cands = lc.make_bow_kf_scene(1)
    kf1.keys["angle"] = 1000.0
    rc, _, _ = search_kf(kf1, cands[:1], 0.75, True)
    assert rc == VIEO_E_INVALID and lib().bw_error() == b"SearchByBoW(KF, KF): key angles outside [0, 360)"


# ---------------------------------------------------------------------------------------------------------------------
def _mask_of(keep):
    m = ALL_BINS
    for i in keep:
        if i >= 0:
            m &= ~(1 << i)
    return m


def _three_maxima(counts):
    c = np.ascontiguousarray(counts, np.int32)
    assert len(c) == reloc_ref.HISTO_LENGTH
    return lib().bw_three_maxima(p(c))


def _bins(**at):
    c = np.zeros(reloc_ref.HISTO_LENGTH, np.int32)
    for k, v in at.items():
        c[int(k[1:])] = v
    return c


def test_three_maxima_against_the_restatement():
    cases = [_bins(), _bins(b7=5), _bins(b0=1), _bins(b29=3),
             _bins(b3=4, b9=4), _bins(b9=4, b3=4, b20=4), _bins(b0=2, b1=2, b2=2, b3=2),  # equal counts: the earlier bin wins
             _bins(b2=10, b5=1), _bins(b5=10, b2=1), _bins(b2=100, b5=10), _bins(b2=100, b5=9), _bins(b5=100, b2=9),
             _bins(b1=30, b4=3, b8=2), _bins(b8=30, b4=3, b1=2), _bins(b1=30, b4=2, b8=3), _bins(b4=3, b1=2, b8=30)]
    rng = np.random.default_rng(3)
    for _ in range(3000):
        c = rng.integers(0, rng.choice([2, 4, 12, 200]), reloc_ref.HISTO_LENGTH)
        c[rng.random(reloc_ref.HISTO_LENGTH) < rng.choice([0.0, 0.5, 0.9])] = 0
        cases.append(c)
    for c in cases:
        assert _three_maxima(c) == _mask_of(reloc_ref.three_maxima([int(v) for v in c])), c
    assert _three_maxima(_bins()) == ALL_BINS  # no bin kept
    assert _three_maxima(_bins(b2=100, b5=10)) == ALL_BINS & ~(1 << 2) & ~(1 << 5)  # 10 is not below a tenth of 100
    assert _three_maxima(_bins(b2=100, b5=9)) == ALL_BINS & ~(1 << 2)
    assert _three_maxima(_bins(b1=30, b4=3, b8=2)) == ALL_BINS & ~(1 << 1) & ~(1 << 4)


def _rot_bin_restated(a1, a2):
    """reloc_ref._bow_walk's statement, without its assertion"""
    factor = f32(1.0) / f32(reloc_ref.HISTO_LENGTH)
    rot = f32(a1) - f32(a2)
    if rot < 0.0:
        rot = f32(rot + f32(360.0))
    b = int(math.floor(float(f32(rot * factor)) + 0.5))
    return 0 if b == reloc_ref.HISTO_LENGTH else b


def test_rot_bin_against_the_restatement():
    below = float(np.nextafter(f32(360.0), f32(0.0)))
    pairs = [(0.0, 0.0), (10.0, 10.0), (below, below), (10.0, 200.0), (0.0, below), (0.0, 0.001), (100.0, 100.5),
             (below, 0.0), (359.99, 0.0), (345.0, 0.0), (350.0, 5.0), (0.0, 15.0)]
    for k in range(12):  # the half-bin boundaries, reached from both sides of the wrap, and their float neighbours
        edge = f32(30 * k + 15)
        for d in (edge, np.nextafter(edge, f32(0)), np.nextafter(edge, f32(1000))):
            pairs += [(float(d), 0.0), (0.0, float(f32(360.0) - d)), (float(d) / 2 + 100.0, 100.0 - float(d) / 2)]
    pairs += [(900.0, 0.0), (885.0, 0.0), (914.0, 0.0), (884.0, 0.0), (916.0, 0.0)]  # bin == HISTO_LENGTH -> 0, and beside it
    rng = np.random.default_rng(4)
    pairs += [tuple(v) for v in rng.uniform(0, 360, (2000, 2)).astype(np.float32).tolist()]
    seen = set()
    for a1, a2 in pairs:
        got = lib().bw_rot_bin(a1, a2)
        assert got == _rot_bin_restated(a1, a2), (a1, a2)
        seen.add(got)
    assert lib().bw_rot_bin(345.0, 0.0) == 12 and lib().bw_rot_bin(15.0, 0.0) == 1 and lib().bw_rot_bin(900.0, 0.0) == 0
    assert lib().bw_rot_bin(0.0, 15.0) == 12  # 345 again, through the wrap: round half away from zero
    assert seen >= set(range(13))


# ---------------------------------------------------------------------------------------------------------------------
def _table_ok(n_keys, ids, first, feat):
    ids, first, feat = np.array(ids, np.uint32), np.array(first, np.int32), np.array(feat, np.int32)
    return lib().bw_node_table_ok(n_keys, len(ids), p(ids), p(first), p(feat))


@pytest.mark.parametrize("ids, first, feat, ok", [
    ([3, 8, 9], [0, 2, 2, 4], [0, 4, 1, 2], 1),      # a correct table with an empty node
    ([3, 9, 8], [0, 2, 2, 4], [0, 4, 1, 2], 0),      # descending ids
    ([3, 8, 8], [0, 2, 2, 4], [0, 4, 1, 2], 0),      # an id twice
    ([3, 8, 9], [1, 2, 2, 4], [0, 4, 1, 2], 0),      # node_first[0] != 0
    ([3, 8, 9], [0, 2, 1, 4], [0, 4, 1, 2], 0),      # node_first decreases
    ([3, 8, 9], [0, 2, 2, 4], [0, 5, 1, 2], 0),      # a feature index equal to n_keys
    ([3, 8, 9], [0, 2, 2, 4], [0, -1, 1, 2], 0),     # a negative one
])
def test_node_table_check(ids, first, feat, ok):
    assert _table_ok(5, ids, first, feat) == ok


def test_node_table_check_of_empty_tables():
    assert lib().bw_node_table_ok(5, 0, None, None, None) == 1  # no nodes: no array is looked at
    assert lib().bw_node_table_ok(0, 0, None, None, None) == 1
    assert lib().bw_node_table_ok(5, -1, None, None, None) == 0
    assert _table_ok(5, [3, 8], [0, 0, 0], []) == 1             # nodes without features: node_feat may be null
    ids, first = np.array([3], np.uint32), np.array([0, 1], np.int32)
    assert lib().bw_node_table_ok(5, 1, p(ids), p(first), None) == 0
    assert lib().bw_node_table_ok(5, 1, None, p(first), None) == 0 and lib().bw_node_table_ok(5, 1, p(ids), None, None) == 0


def test_shared_node_enumeration_is_the_intersection_in_order():
    rng = np.random.default_rng(5)
    for trial in range(200):
        a = np.unique(rng.integers(0, 60, rng.integers(0, 30))).astype(np.uint32)
        b = np.unique(rng.integers(0, 60, rng.integers(0, 30))).astype(np.uint32)
        out = np.zeros((max(len(a), 1), 2), np.int32)
        n = lib().bw_shared_nodes(p(a), len(a), p(b), len(b), p(out))
        both = sorted(set(a.tolist()) & set(b.tolist()))
        assert n == len(both)
        assert a[out[:n, 0]].tolist() == both and b[out[:n, 1]].tolist() == both
