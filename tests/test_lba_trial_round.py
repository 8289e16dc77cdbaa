"""The per-trial round of the local BA (lba_schur_device.h, lba_solve_device.h): k_lba_schur computes and stores only
the 16 x 16 blocks of a diagonal tile that somebody reads -- (i, j) with i <= j, rows below the tile's last valid row,
columns up to column npv -- dealt over the four wavefronts; k_lba_ldlt16 forms the reduced system in its load phase, through the entry functions
k_lba_assemble runs for the larger solver classes, instead of reading an assembled Hs.  No sum changes, so not one bit of
a result may move.

Each case (tests/golden/lba_trial_cases.py) puts column npv, the padding and the tile count somewhere else, or takes
another solver class or call form; each is compared
  * bytewise against tests/golden/lba_trial_<case>.npz -- states, points, erase flags, trial and iteration counts, chi2
    as the commit before the block rule computed them on an MI355X (make_lba_trial_golden.py), and
  * against the CPU oracle at the tolerances of tests/test_lba_xf_table.py, erase flags and LM trial counts equal.
The device result and the oracle's are computed once per case and shared."""
import functools
import os

import numpy as np
import pytest

from tests.golden import lba_trial_cases as cases
from vieo_slam_amd import synth_ba

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def _case(name):
    wins = cases.build(name)
    return wins, cases.run_hip(name, wins)


def _vs_oracle(name, win, h, o):
    """tests/test_lba_xf_table.py::_vs_oracle"""
    kind = cases.CASES[name]["kind"]
    kfs = win[1]
    assert int(h["res"]["status"]) == int(o["res"]["status"]) == 0
    for k in range(len(kfs)):
        dt, dr = synth_ba.pose_error(o["navs"][k], h["navs"][k])
        assert dt < 1e-4 and dr < 1e-4, (name, k, dt, dr)
        if kind != "vision":
            assert np.linalg.norm(o["navs"][k]["v"] - h["navs"][k]["v"]) < 1e-4
            assert np.linalg.norm(o["navs"][k]["dbg"] - h["navs"][k]["dbg"]) < 1e-6
            assert np.linalg.norm(o["navs"][k]["dba"] - h["navs"][k]["dba"]) < 1e-5
    d = np.abs(o["pts"] - h["pts"])
    assert d.max() < 5e-2 and np.median(d) < 2e-5, (name, d.max(), np.median(d))
    assert np.array_equal(o["erase"], h["erase"])
    assert int(h["res"]["lm_trials"]) == int(o["res"]["lm_trials"])
    assert abs(h["res"]["chi2_final"] - o["res"]["chi2_final"]) < 1e-5 * o["res"]["chi2_final"] + 1e-2
    assert abs(h["res"]["chi2_initial"] - o["res"]["chi2_initial"]) < 1e-5 * o["res"]["chi2_initial"]
    if kind == "scale":
        assert abs(o["scale"] - h["scale"]) < 1e-6 and abs(h["scale"] - 1.0) > 1e-4, (o["scale"], h["scale"])


def test_lba_trial_cases_have_the_shapes_they_are_for():
    """point counts as pinned (ragged chunks, the full BA's idle splits), npv and n where the block rule and the solver
    classes turn"""
    npv, n = {}, {}
    for name, c in cases.CASES.items():
        wins = cases.build(name)
        assert [len(w[2]) for w, _ in wins] == cases.N_POINTS[name], name
        nf = int((wins[0][0][1]["fixed"] == 0).sum())
        sco = 1 if c["kind"] == "scale" else 0
        npv[name], n[name] = 6 * nf + sco, (6 if c["kind"] == "vision" else 15) * nf + sco
    assert [npv[k] for k in ("kf1", "kf2", "kf3", "kf6", "kf8", "kf10")] == [6, 12, 18, 36, 48, 60]
    assert (npv["vis11"], npv["vis26"], n["vis26"], n["large11"], npv["scale"]) == (66, 156, 156, 165, 37)
    assert n["kf10"] == 150 and n["vis26"] < 160 <= n["large11"]  # classes 0 and 1
    assert sum(p % 16 != 0 for ps in cases.N_POINTS.values() for p in ps) >= 1
    chunks = (cases.N_POINTS["scale"][0] + 15) // 16  # the full BA: ksplit = min(chunks, 16), cps = ceil(chunks / ksplit)
    ksplit = min(chunks, 16)
    cps = (chunks + ksplit - 1) // ksplit
    assert (ksplit - 1) * cps >= chunks, "no split of the scale case returns early"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cases.CASES))
def test_gpu_lba_trial_round_bytes_equal_parent(name):
    wins, recs = _case(name)
    got = cases.pack(recs)
    with np.load(os.path.join(GOLDEN, "lba_trial_%s.npz" % name)) as want:
        assert sorted(want.files) == sorted(got)
        for k in want.files:
            assert want[k].dtype == got[k].dtype and want[k].shape == got[k].shape, k
            assert want[k].tobytes() == got[k].tobytes(), (name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cases.CASES))
def test_gpu_lba_trial_round_matches_oracle(oracle, name):
    wins, recs = _case(name)
    for (win, _), h, o in zip(wins, recs, cases.run_oracle(oracle, name, wins)):
        _vs_oracle(name, win, h, o)


@pytest.mark.gpu
def test_gpu_lba_trial_round_rejected_trial():
    """kf10: a rejected trial is an LM iteration with more than one lambda trial -- the reduced system formed again with
    only lambda changed -- and an accepted one lowers chi2"""
    res = _case("kf10")[1][0]["res"]
    assert int(res["status"]) == 0
    assert int(res["lm_trials"]) > int(res["lm_iterations"]), "no rejected trial"
    assert res["chi2_final"] < res["chi2_initial"], "no accepted trial"


@pytest.mark.gpu
def test_gpu_lba_trial_round_alone_and_first_of_six():
    """kf3 alone (fused build, one-launch tail) and first of a batch of six with a class-1 window in it (separate
    launches, an assembly loop per class): the poses agree to rounding (the trial's chi2 is summed in another fixed
    order in the one-launch tail), erase flags and trial counts are equal"""
    a, c = _case("kf3")[1][0], _case("six")[1][0]
    for k in range(len(a["navs"])):
        dt, dr = synth_ba.pose_error(a["navs"][k], c["navs"][k])
        assert dt < 1e-6 and dr < 1e-6
    assert np.array_equal(a["erase"], c["erase"]) and int(a["res"]["lm_trials"]) == int(c["res"]["lm_trials"])
