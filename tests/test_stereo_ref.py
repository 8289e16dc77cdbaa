"""The numpy restatement of Frame::ComputeStereoMatches (tests/stereo_ref.py) against the CPU oracle (oracle/matching.cc),
bit for bit, on extracted frames and on every planted frame of tests/stereo_cases.py; the planted frames assert from
the restatement's census that they reach the branches they are named for.  No GPU."""
import numpy as np
import pytest

from tests import stereo_cases, stereo_ref
from vieo_slam_amd import synth

BF, BASELINE = synth.EUROC_BF, synth.EUROC_BF / synth.EUROC_FX
SIZES = [(239, 239), (244, 241)]


def planes(ext):
    return [ext.plane(l, 0) for l in range(ext.nlevels)]


def run_both(oracle, oL, oR, kl, dl, kr, dr, baseline, bf):
    our, odp = oracle.stereo_match(oL, oR, kl, dl, kr, dr, baseline, bf)
    sc = np.array(oL.scale_factors(), np.float32)
    inv = (np.float32(1.0) / sc).astype(np.float32)
    ur, dp, census = stereo_ref.compute_stereo_matches(planes(oL), planes(oR), kl, dl, kr, dr, sc, inv, baseline, bf)
    assert np.array_equal(our.view(np.uint32), ur.view(np.uint32))
    assert np.array_equal(odp.view(np.uint32), dp.view(np.uint32))
    return ur, dp, census


def planted(oracle, frame):
    """(oracle extractors that hold the frame's pyramids, uright, depth, census), the restatement checked on the way"""
    oL, oR = oracle.extractor(300), oracle.extractor(300)
    oL(frame.left), oR(frame.right)
    assert np.array_equal(np.array(oL.scale_factors(), np.float32), frame.scale)
    assert [oL.level_size(l) for l in range(8)] == frame.sizes
    ur, dp, census = run_both(oracle, oL, oR, frame.kl, frame.dl, frame.kr, frame.dr, stereo_cases.BASELINE, stereo_cases.BF)
    return oL, oR, ur, dp, census


@pytest.mark.parametrize("seed", [1000, 1001, 1002])
def test_restatement_extracted_frames(oracle, seed):
    left, right, _ = synth.synth_stereo_pair(seed)
    oL, oR = oracle.extractor(1200), oracle.extractor(1200)
    _, kl, dl = oL(left)
    _, kr, dr = oR(right)
    ur, _, census = run_both(oracle, oL, oR, kl, dl, kr, dr, BASELINE, BF)
    assert (ur >= 0).sum() > 300 and census.count("accepted") == (ur >= 0).sum()


@pytest.mark.parametrize("w,h,n_l,n_r,n_matched", [(239, 239, 303, 302, 187), (244, 241, 305, 304, 202)])
def test_restatement_small_frames(oracle, w, h, n_l, n_r, n_matched):
    left, right, _ = synth.synth_stereo_pair(3000, w, h)
    oL, oR = oracle.extractor(300), oracle.extractor(300)
    _, kl, dl = oL(left)
    _, kr, dr = oR(right)
    ur, _, census = run_both(oracle, oL, oR, kl, dl, kr, dr, BASELINE, BF)
    assert (len(kl), len(kr), int((ur >= 0).sum())) == (n_l, n_r, n_matched)
    print(census.gates(), "candidates per row up to", max(r["n_cand"] for r in census))


@pytest.mark.parametrize("w,h", SIZES)
def test_planted_frames(oracle, w, h):
    gates = {}
    for frame in stereo_cases.all_frames(w, h):
        _, _, _, _, census = planted(oracle, frame)
        frame.check(census)
        for g, n in census.gates().items():
            gates[g] = gates.get(g, 0) + n
    print(gates)
    assert all(gates[g] > 0 for g in stereo_ref.GATES if g != "deltaR"), gates  # (the deltaR gate cannot close: stereo_cases)


def test_planted_tall_frame(oracle):
    frame = stereo_cases.frame_tall(640, 1030)
    _, _, _, _, census = planted(oracle, frame)
    frame.check(census)
    assert max(r["row"] for r in census) == 1029 and sum(r["row"] >= 1023 and r["gate"] == "accepted" for r in census) == 2


@pytest.mark.parametrize("w,h", [(260, 600), (560, 1030)])
def test_oracle_extractor_refuses_too_tall(oracle, w, h):
    """round(regionW / regionH) == 0 at some level: DistributeOctTree has no root node (the library refuses the same
    shapes); 640 x 1030 is inside the domain"""
    with pytest.raises(ValueError, match="too tall"):
        oracle.extractor(300)(synth.synth_image(5, w, h))


def test_oracle_extractor_accepts_tall(oracle):
    _, kps, _ = oracle.extractor(300)(synth.synth_image(5, 640, 1030))
    assert len(kps) > 200
