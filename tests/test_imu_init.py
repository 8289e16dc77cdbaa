"""vieo_imu_init on the device against the restatement of IMUInitialization::TryInitVIO (tests/imu_init_ref.py).

Parity: every result field, per-key-frame output and point.  The restatement takes its pre-integrations from the device's
own vieo_imu_preintegrate_batch (tested on its own against the oracle), so what is compared is the new steps.  Tolerance
(tests/imu_init_ref.tolerance): the device's distance from the 50-digit evaluation may be 16 x d_ref, d_ref = the float64
restatement's distance from the same 50-digit value, with a floor of 1e-13 relative to the field's largest magnitude; the
distance to the float_rows restatement (what the reference's CV_32F arithmetic would print) is printed, not asserted.
Shapes: N = 6 (the smallest that passes the gate), 66 and 67 (64 and 65 triples: one wavefront of triples and one past it),
one case at the cap of 512 key frames."""
import functools

import numpy as np
import pytest

from tests import imu_init_ref as ref
from vieo_slam_amd import _lib, imu
from vieo_slam_amd import imu_init as ii

pytestmark = pytest.mark.gpu

RESULT_FIELDS = ("bg", "s_star", "gw_star", "w", "RwI", "s", "dtheta", "ba", "w2", "RwI_opt", "gw")
CASES = {
    "n6": lambda: ii.make_init_case(3, 6),
    "n21": lambda: ii.make_init_case(3, 21),
    "n66": lambda: ii.make_init_case(3, 66, step=2),
    "n67": lambda: ii.make_init_case(3, 67, step=2),
    "hole": lambda: ii.make_init_case(3, 12, empty=(5,)),       # an interval without samples in the middle
    "grown": lambda: ii.make_init_case(3, 12, n_kf_init=9),     # n_kf = n_kf_init + 3
    "closed": lambda: ii.make_init_case(3, 12, apply=0),
    "few_kf": lambda: ii.make_init_case(3, 3),
    "few_eq": lambda: ii.make_init_case(3, 5),
    "degenerate": lambda: ii.make_static_case(6),
    "cap": lambda: ii.make_init_case(5, ii.MAX_KF, step=1, s_true=1.7),
}


def _device_preintegrate(noise, lists, ti, tj, bg, ba):
    return imu.imu_preintegrate(noise, lists, ti, tj, bg, ba)


@functools.lru_cache(maxsize=None)
def _case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def _refs(name):
    """(float64 restatement, 50-digit evaluation, float_rows restatement): computed once, shared, never changed"""
    c = _case(name)
    R = ref.restate(c, preintegrate=_device_preintegrate)
    return R, ref.restate(c, arith="mp", shared=R), ref.restate(c, float_rows=True, shared=R)


@functools.lru_cache(maxsize=None)
def _alone(name):
    return ii.try_init_vio([_case(name)])[0]


def _bytes(o):
    return b"".join(np.ascontiguousarray(o[k]).tobytes() for k in ("result", "Tcw", "nav", "nav_set", "preint", "sigma_prv", "points"))


def _close(what, got, r64, r50, rf=None):
    tol, d_ref = ref.tolerance(r64, r50)
    d = ref.dist(got, r50)
    print("%-18s d_ref %.2e tol %.2e device %.2e%s" % (what, d_ref, tol, d, "" if rf is None else
                                                       "  (float_rows: %.2e)" % ref.dist(got, rf)))
    assert d <= tol, what


def _check(name, o):
    c = _case(name)
    R, R50, Rf = _refs(name)
    r = o["result"]
    print("%s: status %d sweeps %s" % (name, r["status"], r["sweeps"]))
    assert (r["status"], r["n_eq_gyro"], r["n_eq"], r["inited"]) == (R["status"], R["n_eq_gyro"], R["n_eq"], R["inited"])
    if R["status"] == ii.FEW_KF:
        live = ()
    elif R["status"] == ii.FEW_EQUATIONS:
        live = ("bg",)
    elif R["status"] == ii.DEGENERATE_GRAVITY:  # (s* lies along a singular direction the rule raised: not defined)
        live = ("bg", "gw_star", "w")
    else:
        live = RESULT_FIELDS
        assert all(1 <= s < ii.MAX_SWEEPS for s in r["sweeps"])
    for f in RESULT_FIELDS:
        if f in live:
            _close(f, r[f], R[f], R50[f], Rf.get(f))
        elif not (R["status"] == ii.DEGENERATE_GRAVITY and f == "s_star"):
            assert not np.any(r[f]), f
    n_kf = len(c["Twc"])
    if not R["inited"]:  # nothing of step 5 is written
        for k in ("Tcw", "nav", "nav_set", "preint", "sigma_prv", "points"):
            assert not np.frombuffer(np.ascontiguousarray(o[k]).tobytes(), np.uint8).any(), k
        return
    assert np.array_equal(o["nav_set"], R["nav_set"])
    _close("Tcw", o["Tcw"], R["Tcw"], R50["Tcw"], Rf["Tcw"])
    on = o["nav_set"] == 1
    nav = o["nav"]
    assert not np.frombuffer(nav[~on].tobytes(), np.uint8).any()  # the `continue`: the record stays zero
    for f, g in (("p", "nav_p"), ("q", "nav_q"), ("v", "nav_v")):
        _close("nav." + f, nav[f][on], R[g][on], R50[g][on], Rf[g][on])
    assert np.array_equal(nav["bg"][on], np.tile(r["bg"], (on.sum(), 1))) and np.array_equal(nav["ba"][on], np.tile(r["ba"], (on.sum(), 1)))
    assert not nav["dbg"].any() and not nav["dba"].any()
    # the points: float products by (float)s; s itself is within its tolerance, so allow the last bit of (float)s
    sf = np.float32(r["s"])
    assert np.array_equal(o["points"]["pos"], c["points"]["pos"] * sf)
    assert np.array_equal(o["points"]["max_dist"], c["points"]["max_dist"] * sf)
    assert np.array_equal(o["points"]["min_dist"], c["points"]["min_dist"] * sf)
    assert abs(float(sf) - float(np.float32(float(R["s"])))) <= np.spacing(sf)
    assert len(o["preint"]) == n_kf


@pytest.mark.parametrize("name", ["n6", "n66", "n67", "hole", "grown", "closed", "few_kf", "few_eq", "degenerate"])
def test_parity_with_the_restatement(name):
    _check(name, _alone(name))


def test_the_hole_leaves_its_predecessor_unset():
    o = _alone("hole")
    assert list(np.flatnonzero(o["nav_set"] == 0)) == [4] and o["Tcw"][4].any()
    assert o["result"]["n_eq"] == 12 - 4 and o["result"]["n_eq_gyro"] == 12 - 2


def test_batch_invariance():
    names = ["n6", "n67", "n21"]
    alone = {n: _bytes(_alone(n)) for n in names}
    for rot in range(3):  # every sequence first, in the middle and last of three
        order = names[rot:] + names[:rot]
        out = ii.try_init_vio([_case(n) for n in order])
        for n, o in zip(order, out):
            assert _bytes(o) == alone[n], (order, n)
    again = ii.try_init_vio([_case(n) for n in names])
    assert [_bytes(o) for o in again] == [alone[n] for n in names]  # run to run
    for bad in ("few_kf", "few_eq", "degenerate"):  # a non-OK sequence in the middle changes nothing for its neighbours
        out = ii.try_init_vio([_case("n6"), _case(bad), _case("n67")])
        assert _bytes(out[0]) == alone["n6"] and _bytes(out[2]) == alone["n67"]
        assert out[1]["result"]["status"] == _refs(bad)[0]["status"] and _bytes(out[1]) == _bytes(_alone(bad))


@pytest.mark.parametrize("name", ["n6", "n67", "hole", "grown"])
def test_the_returned_preintegrations_are_the_batch_entrys(name):
    c, o = _case(name), _alone(name)
    n = len(c["Twc"])
    t = np.asarray(c["t"])
    ti, tj = np.concatenate([t[:1], t[:-1]]), t
    pre, prv, _ = imu.imu_preintegrate(c["noise"], c["samples"], ti, tj, np.tile(o["result"]["bg"], (n, 1)),
                                       np.tile(o["result"]["ba"], (n, 1)))
    assert pre.tobytes() == o["preint"].tobytes() and prv.tobytes() == o["sigma_prv"].tobytes()


def test_the_stored_preintegrations_may_be_passed_in():
    c = dict(_case("n21"))
    t = np.asarray(c["t"])
    z = np.zeros((len(t), 3))
    c["preint"], c["preint_sigma_prv"], _ = imu.imu_preintegrate(c["noise"], c["samples"], np.concatenate([t[:1], t[:-1]]), t, z, z)
    assert _bytes(ii.try_init_vio([c])[0]) == _bytes(_alone("n21"))


def test_the_cap():
    _check("cap", _alone("cap"))
    c = ii.make_init_case(5, ii.MAX_KF + 1, step=1, s_true=1.7)
    rc, _ = ii.try_init_vio([c], raw=True)
    assert rc == _lib.VIEO_E_INVALID
    rc, out = ii.try_init_vio([_case("n6"), c], raw=True)  # nothing is launched for its neighbour either
    assert rc == _lib.VIEO_E_INVALID and out[0]["result"]["status"] == 0 and not out[0]["Tcw"].any()


def test_a_batch_of_256():
    protos = [ii.make_init_case(3 + k, 6) for k in range(8)]
    alone = [_bytes(ii.try_init_vio([p])[0]) for p in protos]
    out = ii.try_init_vio([protos[b % 8] for b in range(ii.MAX_SEQ)])
    assert len(out) == ii.MAX_SEQ
    for b, o in enumerate(out):
        assert _bytes(o) == alone[b % 8], b
        assert o["result"]["status"] == ii.OK and o["result"]["inited"] == 1
    rc, _ = ii.try_init_vio([protos[0]] * (ii.MAX_SEQ + 1), raw=True)
    assert rc == _lib.VIEO_E_INVALID
