"""The pose graph without a GPU: the CPU reference (tests/pose_graph_ref.py) against closed forms, so that it does not
certify itself; the device's Sim3 header (csrc/sim3_device.h) compiled for the host against that reference; the golden
file against a regeneration of its smallest case; and essential_graph_edges on hand-built maps with known answers."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from tests import pose_graph_ref as R
from tests.golden import make_pose_graph_golden as gen
from vieo_slam_amd import pose_graph as pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pose_graph_golden.npz")

# twists over all four branches of exp and log: theta below / above eps = 1e-5 (log switches on d > 1 - eps, i.e. at
# theta = 4.47e-3), sigma below / above eps
BRANCH_TWISTS = [[th * a for a in (0.6, -0.48, 0.64)] + [0.3, -1.2, 2.0, sg]
                 for th in (0.0, 3e-6, 1e-4, 4e-3, 5e-3, 0.5, 3.0) for sg in (0.0, 5e-6, -5e-6, 2e-5, 0.1, -0.3)]


def test_log_of_exp_is_the_identity_across_the_branches():
    lm = R.Libm(0)
    for u in BRANCH_TWISTS:
        back = np.array(R.log(R.exp(u, lm), lm))
        # A and B cancel in their numerators: an absolute error of 1e-16 / (theta^2 + sigma^2) in A, next to Omega
        # (theta) and upsilon (2.4): 1e-16 * theta * 2.4 / (theta^2 + sigma^2), below 2.4e-12 / theta.  The eps-branches
        # truncate their series, but exp and log truncate alike.
        # Between theta = 1e-5 and 4.47e-3 exp is exact and log takes its d > 1 - eps branch: omega = 0.5 deltaR is
        # sin(theta) / theta * omega, theta^3 / 6 = 1.5e-8 off at the switch, and A = 1/2 adds theta^3 / 24 * 2.4.
        th = np.linalg.norm(u[:3])
        assert np.abs(back - np.array(u)).max() < (2.5e-8 if 1e-5 <= th < 4.5e-3 else 1e-9), (u, back)
        # (below 0.5 rad, 1 - d^2 and 1 - cos(theta) lose log2(1 / theta^2) bits; C = (s - 1) / sigma loses 1e-16 / sigma)
        if th >= 0.5 and (u[6] == 0.0 or abs(u[6]) >= 0.1):
            assert np.abs(back - np.array(u)).max() < 1e-12, (u, back)


def test_product_with_the_inverse_is_the_identity():
    lm = R.Libm(0)
    for u in BRANCH_TWISTS:
        S = R.exp(u, lm)
        for P in (R.mul(S, R.inverse(S)), R.mul(R.inverse(S), S)):
            assert np.abs(np.array(P[0]) - [0, 0, 0, 1]).max() < 1e-15
            assert np.abs(np.array(P[1])).max() < 1e-14 and abs(P[2] - 1) < 1e-15
        p = [0.3, -2.0, 5.0]
        assert np.abs(np.array(R.smap(R.inverse(S), R.smap(S, p))) - p).max() < 1e-14


def test_two_vertex_graph_reaches_zero():
    c = gen.case_two_kf()
    out = gen.run(c, 0)
    assert out["chi2_initial"] > 0.1 and out["chi2_final"] < 1e-24
    S0, S1 = R.from_record(c["Scw"][0]), out["est"][1]
    P0, P1 = R.from_record(c["Scw_prior"][0]), R.from_record(c["Scw_prior"][1])
    # e = log(C S1 S0^-1) = 0 with C = P0 P1^-1  <=>  S1 = C^-1 S0 = P1 P0^-1 S0
    want = R.mul(R.mul(P1, R.inverse(P0)), S0)
    assert max(R.pose_distance(S1, want)) < 1e-12


def test_perturbed_libm_is_deterministic_and_within_one_ulp():
    a, b = R.Libm(3), R.Libm(3)
    moved = 0
    for k in range(200):
        x = 0.01 + 0.013 * k
        assert a.sin(x) == b.sin(x)
        assert abs(a.sin(x) - math.sin(x)) <= math.ulp(math.sin(x))
        moved += a.sin(x) != math.sin(x)
    assert 60 < moved < 140  # (half of the arguments, by the hash)


def test_smallest_golden_case_regenerates():
    g = np.load(GOLDEN)
    c, m = gen.smallest_case()
    assert np.array_equal(g["two_kf/Scw"], gen.flat(c["Scw"])) and np.array_equal(g["two_kf/Scw_prior"], gen.flat(c["Scw_prior"]))
    assert np.array_equal(g["two_kf/est"], m["est"]) and np.array_equal(g["two_kf/trace"], m["trace"])
    assert int(g["two_kf/lm_trials"]) == m["lm_trials"] and float(g["two_kf/chi2_final"]) == m["chi2_final"]


def test_golden_cases_keep_the_generators_conditions():
    g = np.load(GOLDEN)
    for name in ("ring24", "ring_holes", "kf40", "scale16", "isolated", "reject"):
        assert float(g[name + "/pose_spread"]) <= 1e-5, name
        assert int(g[name + "/n_leading"]) >= 2 and len(g[name + "/chi_spread"]) == int(g[name + "/n_leading"]), name
    lead = int(g["reject/n_leading"])
    assert (g["reject/trace"][:lead, 3] == 0).any() and (g["reject/trace"][:lead, 3] == 1).any()
    assert int(g["ring24/n_unknowns"]) == 138 and int(g["scale16/n_unknowns"]) == 105
    info = g["kf40/edge_info"]
    assert (info == [0.25, 0.5]).all(axis=1).sum() == 1
    pairs = list(zip(g["kf40/edge_i"], g["kf40/edge_j"]))
    assert len(pairs) > len(set(pairs))  # a duplicate (i, j)


@pytest.fixture(scope="module")
def host_sim3(tmp_path_factory):
    """csrc/sim3_device.h compiled for the host (the arithmetic the kernels run, without -ffast-math or contraction)"""
    d = tmp_path_factory.mktemp("sim3")
    src = d / "sim3_host.cc"
    src.write_text('#include "sim3_device.h"\nusing namespace vieo;\nextern "C" {\n'
                   "void h_exp(const double* u, Sim3* o) { *o = s3_exp(u); }\n"
                   "void h_log(const Sim3* s, double* o) { s3_log(*s, o); }\n"
                   "void h_err(const Sim3* c, const Sim3* a, const Sim3* b, double* o) { s3_edge_error(*c, *a, *b, o); }\n}\n")
    so = str(d / "libsim3_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I",
                           os.path.join(ROOT, "vieo_slam_amd", "csrc"), str(src), "-o", so])
    return ctypes.CDLL(so)


def test_device_header_on_the_host_agrees_with_the_reference(host_sim3):
    lm = R.Libm(0)
    rng = np.random.default_rng(3)
    for u in BRANCH_TWISTS:
        ua = np.array(u, np.float64)
        S = np.zeros(1, pg.SIM3_DTYPE)
        host_sim3.h_exp(ua.ctypes.data_as(ctypes.c_void_p), S.ctypes.data_as(ctypes.c_void_p))
        want = R.exp(u, lm)
        got = R.from_record(S[0])
        assert np.abs(np.array(got[0]) - want[0]).max() < 1e-15 and np.abs(np.array(got[1]) - want[1]).max() < 1e-14
        back = np.zeros(7)
        host_sim3.h_log(S.ctypes.data_as(ctypes.c_void_p), back.ctypes.data_as(ctypes.c_void_p))
        assert np.abs(back - np.array(R.log(got, lm))).max() < 1e-13
        A = R.to_records([R.exp(list(rng.standard_normal(7) * 0.4), lm) for _ in range(2)], pg.SIM3_DTYPE)
        e = np.zeros(7)
        host_sim3.h_err(S.ctypes.data_as(ctypes.c_void_p), A[0:1].ctypes.data_as(ctypes.c_void_p),
                        A[1:2].ctypes.data_as(ctypes.c_void_p), e.ctypes.data_as(ctypes.c_void_p))
        assert np.abs(e - np.array(R.edge_error(got, R.from_record(A[0]), R.from_record(A[1]), lm))).max() < 1e-12


# ---------------------------------------------------------------------------------------------------------------------
def _edges(*a, **k):
    ei, ej, kind, info = pg.essential_graph_edges(*a, **k)
    return [(int(i), int(j), int(c), tuple(float(v) for v in w)) for i, j, c, w in zip(ei, ej, kind, info)]


def _chain_cov(n, w=200, extra=()):
    """key frame k sees k - 1 with weight w (both directions), plus extra (i, j, w) rows in both directions"""
    rows = {}
    for k in range(1, n):
        rows.setdefault(k, []).append((k - 1, w))
        rows.setdefault(k - 1, []).append((k, w))
    for i, j, ww in extra:
        rows.setdefault(i, []).append((j, ww))
        rows.setdefault(j, []).append((i, ww))
    return [(i, j, ww) for i in sorted(rows) for j, ww in sorted(rows[i], key=lambda r: -r[1])]


ONE = (1.0, 1.0)


def test_edges_of_a_chain_with_one_loop():
    n = 6
    parent = np.arange(-1, n - 1)
    got = _edges(np.ones(n), parent, [], _chain_cov(n), {5: [0]}, 5, 0)
    # the (cur, loop) pair enters although the two share no map point; then one spanning-tree edge per key frame
    assert got == [(5, 0, 0, ONE)] + [(k, k - 1, 1, ONE) for k in range(1, n)]


def test_edges_weight_99_against_100_and_the_cur_loop_exception():
    n = 6
    parent = np.arange(-1, n - 1)
    cov = _chain_cov(n, extra=[(5, 1, 99), (4, 0, 100), (4, 2, 99), (5, 2, 100)])
    got = _edges(np.ones(n), parent, [], cov, {5: [0, 1], 4: [0]}, 5, 0)
    # loop connections in nid_ order: (4, 0) has 100 -> kept; (5, 0) is the exception; (5, 1) has 99 -> dropped
    assert got[:2] == [(4, 0, 0, ONE), (5, 0, 0, ONE)]
    rest = got[2:]
    # covisibility: (4, 2) has 99 -> no edge; (5, 2) has 100 -> edge; (4, 0) is a new loop connection already -> not again
    assert (5, 2, 1, ONE) in rest and (4, 2, 1, ONE) not in rest and (4, 0, 1, ONE) not in rest and (5, 1, 1, ONE) not in rest
    assert [e for e in rest if e[:2] not in ((5, 2),)] == [(k, k - 1, 1, ONE) for k in range(1, n)]


def test_edges_duplicate_loop_connection_and_covisibility_pair():
    n = 6
    parent = np.arange(-1, n - 1)
    cov = _chain_cov(n, extra=[(5, 1, 150), (4, 1, 150)])
    # (5, 1) and (1, 5) are both loop connections: both are added (the reference adds per ordered pair) and the
    # covisibility pair (5, 1) is then left out; (4, 1) is an ordinary covisibility edge, added once, from the higher id
    got = _edges(np.ones(n), parent, [], cov, {5: [0, 1], 1: [5]}, 5, 0)
    assert got[:3] == [(1, 5, 0, ONE), (5, 0, 0, ONE), (5, 1, 0, ONE)]
    assert got.count((4, 1, 1, ONE)) == 1 and (1, 4, 1, ONE) not in got and (5, 1, 1, ONE) not in got


def test_edges_parent_that_is_a_loop_connection_is_kept_twice():
    n = 4
    parent = np.array([-1, 0, 1, 0])  # key frame 3's parent is the loop key frame 0
    cov = _chain_cov(3) + [(3, 0, 300), (0, 3, 300)]
    got = _edges(np.ones(n), parent, [], cov, {3: [0]}, 3, 0)
    assert got == [(3, 0, 0, ONE), (1, 0, 1, ONE), (2, 1, 1, ONE), (3, 0, 1, ONE)]


def test_edges_has_child_parent_and_old_loop_exclusions():
    n = 6
    parent = np.array([-1, 0, 1, 2, 1, 4])  # 4 is a child of 1
    cov = _chain_cov(n, extra=[(4, 1, 400), (5, 2, 300), (5, 3, 250)])
    loops = [(5, 2), (2, 5)]  # an old loop edge 5 - 2
    got = _edges(np.ones(n), parent, loops, cov, {}, 5, 0)
    # 4 -> 1 is the spanning-tree edge of 4, so the covisibility pair (4, 1) adds nothing (parent for 4, hasChild for 1);
    # 5 -> 2 is the old loop edge (towards the lower id only), so its covisibility pair adds nothing; 5 -> 3 is added
    assert got.count((4, 1, 1, ONE)) == 1 and got.count((5, 2, 1, ONE)) == 1 and (2, 5, 1, ONE) not in got
    assert got.count((5, 3, 1, ONE)) == 1
    # 4 sees 3 with 200 (its chain row) and 3 is neither parent nor child nor loop edge of 4: a covisibility edge
    assert got.count((4, 3, 1, ONE)) == 1 and (3, 4, 1, ONE) not in got


def test_edges_bad_key_frame_and_order():
    n = 5
    valid = np.array([1, 1, 0, 1, 1])
    parent = np.array([-1, 0, -1, 1, 3])
    cov = [(1, 0, 200), (3, 1, 200), (3, 0, 120), (3, 2, 500), (4, 3, 200), (4, 1, 180), (4, 0, 130)]
    got = _edges(valid, parent, [(4, 0), (0, 4), (4, 1), (1, 4)], cov, {}, 4, 0)
    # per key frame: spanning tree, old loop edges in ascending id, covisibles in the order of their list (by weight);
    # a bad neighbour (3 -> 2) is skipped
    assert got == [(1, 0, 1, ONE), (3, 1, 1, ONE), (3, 0, 1, ONE), (4, 3, 1, ONE), (4, 0, 1, ONE), (4, 1, 1, ONE)]


def test_edges_odometry_information_and_the_carried_matrix():
    n = 6
    parent = np.arange(-1, n - 1)
    cov = [(k, k - 1, 200) for k in range(1, n) if k not in (2, 3, 4)] + [(3, 2, 40)]  # 2, 3, 4: weak spanning-tree edges
    base = {2: (0.5, 0.25), 4: (0.8, 0.1)}   # fOdomBase = (min(1, 0.5, 0.8), min(1, 0.25, 0.1)) = (0.5, 0.1)
    edge = {2: (2.0, 0.5), 4: (1.0, 0.4)}
    got = _edges(np.ones(n), parent, [], cov, {}, 5, 0, odom_sigma_base=base, odom_sigma_edge=edge)
    # key frame 3's edge is weak (weight 40 < 100) but not under the odometry condition: matLambda, whatever
    # matLambdaOdom still holds from key frame 2
    assert got == [(1, 0, 1, ONE), (2, 1, 1, (0.25, float(np.float32(0.1) / np.float32(0.5)))), (3, 2, 1, ONE),
                   (4, 3, 1, (0.5, 0.25)), (5, 4, 1, ONE)]
    # elemInfo == 0 or > 1e6 -> identity block
    got = _edges(np.ones(n), parent, [], cov, {}, 5, 0, odom_sigma_base={2: (0.5, 0.25)}, odom_sigma_edge={2: (1e-9, 0.5)})
    assert got[1] == (2, 1, 1, (1.0, 0.5))


def test_edges_refuse_a_bad_endpoint():
    with pytest.raises(ValueError):
        pg.essential_graph_edges(np.array([1, 0]), np.array([-1, -1]), [], [], {0: [1]}, 0, 1)
