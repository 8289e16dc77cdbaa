"""The restatement of IMUInitialization::TryInitVIO (tests/imu_init_ref.py) on its own, without a GPU: against the truth of
the synthetic sequences (sanity, not parity), the gates, the `continue` rules of the map update, apply = 0 and a key-frame
list that grew after the snapshot."""
import functools

import numpy as np
import pytest

from tests import imu_init_ref as ref
from vieo_slam_amd import imu_init as ii


@functools.lru_cache(maxsize=None)
def _run(seed, n, step=10, s_true=1.0, empty=(), **kw):
    c = ii.make_init_case(seed, n, step, s_true, empty=empty, **kw)
    return c, ref.restate(c)


# The restatement's own errors against the truth, measured when this test was written, doubled:
#   seed N step s_true | bg [rad/s]  gravity direction [rad]  s (relative)  ba [m/s^2]  v [m/s]
#   3    21  10  1     | 1.03e-4     3.13e-3                  1.67e-2       2.87e-2     8.23e-3
#   5    31  10  1.7   | 1.03e-4     6.94e-4                  3.55e-5       4.81e-3     1.91e-3
#   3    6   10  1     | 6.61e-5     (N < 21: the accelerometer bias and with it direction and scale are barely observable)
#   7    12  5   1     | 1.27e-4
@pytest.mark.parametrize("seed,n,step,s_true,bounds", [
    (3, 21, 10, 1.0, dict(bg=2.1e-4, direction=6.3e-3, s=3.4e-2, ba=5.8e-2, v=1.7e-2)),
    (5, 31, 10, 1.7, dict(bg=2.1e-4, direction=1.4e-3, s=7.1e-5, ba=9.7e-3, v=3.9e-3)),
    (3, 6, 10, 1.0, dict(bg=1.4e-4)),
    (7, 12, 5, 1.0, dict(bg=2.6e-4)),
])
def test_the_restatement_finds_the_truth(seed, n, step, s_true, bounds):
    c, R = _run(seed, n, step, s_true)
    tr = c["truth"]
    assert R["status"] == ii.OK and R["n_eq_gyro"] == n - 1 and R["n_eq"] == n - 2 and R["inited"] == 1
    got = dict(bg=np.abs(R["bg"] - tr["bg"]).max(),
               direction=np.arccos(np.clip(R["gw"] @ tr["gw"] / np.linalg.norm(R["gw"]) / np.linalg.norm(tr["gw"]), -1, 1)),
               s=abs(R["s"] / s_true - 1), ba=np.abs(R["ba"] - tr["ba"]).max(), v=np.abs(R["nav_v"] - tr["v"]).max())
    print({k: "%.3g" % v for k, v in got.items()}, "cond(A) %.3g cond(C) %.3g" % (R["w"][0] / R["w"][-1], R["w2"][0] / R["w2"][-1]))
    for k, b in bounds.items():
        assert got[k] <= b, k
    assert abs(np.linalg.norm(R["gw"]) - ii.REF_G) < 1e-12  # gw = RwI_opt gI G
    assert R["nav_set"].all()
    # the scaled poses: Tcw = (Rwc^T | -s Rwc^T pwc), pwb = s pwc + Rwc pcb
    for k in (0, n - 1):
        Twc = c["Twc"][k]
        assert np.allclose(R["Tcw"][k][:, :3], Twc[:, :3].T, atol=0, rtol=0)
        assert np.allclose(R["Tcw"][k][:, 3], -Twc[:, :3].T @ Twc[:, 3] * R["s"], atol=1e-15)
    p = c["points"]
    sf = np.float32(R["s"])
    assert np.array_equal(R["points"]["pos"], p["pos"] * sf) and np.array_equal(R["points"]["max_dist"], p["max_dist"] * sf)


def test_the_gates():
    assert _run(3, 3)[1]["status"] == ii.FEW_KF                       # KeyFramesInMap() < 4
    R = _run(3, 5)[1]
    assert R["status"] == ii.FEW_EQUATIONS and R["n_eq"] == 3 and R["n_eq_gyro"] == 4   # numEquations < 4
    R = _run(3, 6, empty=(3,))[1]                                     # one empty interval takes two of the four triples
    assert R["status"] == ii.FEW_EQUATIONS and R["n_eq"] == 2 and R["n_eq_gyro"] == 4
    R = _run(3, 6)[1]
    assert R["status"] == ii.OK and R["n_eq"] == 4
    assert ref.restate(ii.make_static_case(6))["status"] == ii.DEGENERATE_GRAVITY


def test_an_interval_without_samples_in_the_middle():
    n, hole = 12, 5
    c, R = _run(3, n, empty=(hole,))
    assert R["status"] == ii.OK and R["n_eq_gyro"] == n - 2 and R["n_eq"] == n - 4
    # the triples (hole - 2, hole - 1, hole) and (hole - 1, hole, hole + 1) are skipped: their rows stay zero
    for rows in (R["rows1"], R["rows2"]):
        zero = [i for i in range(n - 2) if not rows[3 * i:3 * i + 3].any()]
        assert zero == [hole - 2, hole - 1]
    # the `continue`: key frame hole - 1 (its successor's interval is empty) keeps its NavState; every other one is set.
    # (the last key frame would be the second one, were its own interval the empty one)
    assert list(np.flatnonzero(R["nav_set"] == 0)) == [hole - 1]
    assert R["Tcw"][hole - 1].any() and not R["nav_p"][hole - 1].any()
    c2, R2 = _run(3, n, empty=(n - 1,))
    assert list(np.flatnonzero(R2["nav_set"] == 0)) == [n - 2, n - 1]  # the last interval: two key frames with nav_set = 0


def test_a_closed_gate_computes_and_applies_nothing():
    c, R = _run(3, 12, apply=0)
    assert R["status"] == ii.OK and R["inited"] == 0 and "Tcw" not in R and not R["nav_set"].any()
    c1, R1 = _run(3, 12)
    for f in ("bg", "s", "ba", "gw", "w2"):
        assert np.array_equal(R[f], R1[f])


def test_a_list_that_grew_after_the_snapshot():
    n, extra = 9, 3
    c, R = _run(3, n + extra, n_kf_init=n)
    c0, R0 = _run(3, n)
    for f in ("bg", "s_star", "gw_star", "w", "s", "dtheta", "ba", "w2", "gw"):  # steps 1-4 see the snapshot alone
        assert np.array_equal(R[f], R0[f]), f
    assert R["nav_set"].all() and len(R["nav_set"]) == n + extra         # step 5 sees the whole list
    assert np.array_equal(R["nav_v"][:n - 1], R0["nav_v"][:n - 1])
    assert not np.array_equal(R["nav_v"][n - 1], R0["nav_v"][n - 1])    # no longer the last key frame: the other formula
