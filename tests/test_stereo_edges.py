"""ComputeStereoMatches on the device at its edges: the planted frames of tests/stereo_cases.py through both entry
points, bit-equal to oracle/matching.cc.  tests/test_stereo_ref.py checks on the host that every frame reaches the
branches it is named for (the census of tests/stereo_ref.py) and that the restatement equals the oracle.

What runs.  22 planted frames at 239 x 239 and at 244 x 241 (host entry: every frame; batch entry: the 244 x 241 ones in a
batch of 17, which takes k_stereo_rows<256>, and one of 16, which takes k_stereo_rows<1024>; every frame is in one of the
two, and both hold the frame without left keys, the one without right keys, the two with more than 2048 left keys and
the one with 65 candidates in a row), and one 640 x 1030 frame (alone, and in batches of 2, 16 and 17 of its size: the
prefix sum of the row kernels takes 2 and 5 rows a thread there).  Every output is compared as uint32 with the oracle's;
a batch frame also with the same frame alone through the host entry; output rows from a frame's count up to the capacity
keep a guard pattern; the batch of 17 gives the same bytes twice.

Cases per branch, from the census (one image size; the other differs only where unpainted pixels decide):
  gate that ended the key   no candidate 20, maxU < 0 1, bestDist >= 75 10 (distances 75, 99, 100 and the octave / column
                            gates that leave nothing), endu >= cols 2 (octave 0 and 2; cols - 1 accepted at both),
                            bestincR = -L 4..8 (planted -5, the flat patch, the checkerboard), bestincR = +L 4,
                            disparity 1..2 (exactly maxD), median 2059..2062, accepted 4624.  deltaR: none -- it cannot
                            close on finite values (tests/stereo_cases.py)
  candidates in the row     1, 16 (2 keys), 17 (3), 20, 32, 33 (4), 40 (2), 49, 64 (2), 65 (5); the winner first, last, and
                            in the middle of the second pass
  ties                      11 keys: 2 to 49 equal best distances; the lowest index in another lane, another pass, and
                            behind the others in the row's list (frame tie_order)
  octaves                   left 0 against right 0, 1, 2 and left 7 against right 5, 6, 7; a closer key two octaves off
  columns                   uR == uL, uR == uL - maxD and one ulp beyond each
  refinement                bestincR -5, -4, +4, +5; SAD 0 at two increments (deltaR = +0.5); dist1 = dist2 + 1 (deltaR
                            just above -0.5); deltaR = 0 (mirror-symmetric strips, 5 keys); disparity 0 -> the 0.01 branch (2 keys),
                            just below maxD (accepted) and at maxD (rejected); SAD sums of 60 x 510 and 120 x 510
  row table                 bands clipped at row 0 and at the last row, an integer y, the 16 rows of octave 7, rows h - 7,
                            h - 6 (the last one a patch fits in) and h - 1 of the 1030-row frame
  median                    0, 1, 2, 3, 4 accepted matches; all equal; median 0 (all rejected); {10, 10, 10, 20, 21, 22};
                            SADs at thDist - 1, thDist, thDist + 1 for medians 10 and 20 (thDist comes out as 21.0 and
                            42.0 in float: 21 and 42 are rejected); 2448 keys whose median is 25 but 10 over the first
                            2048 (nothing rejected / 1348 rejected), 4148 keys whose median is 10 but 30 over the first
                            2048 (2048 rejected / none)

Found: nothing in matching.hip; every frame was bit-equal at the first run.  The oracle's extractor crashed on images
with a pyramid level taller than twice its width; it now returns an error (tests/test_stereo_ref.py, and
test_extractor_refuses_too_tall_then_extracts here for the library's side).

Deliberate faults in matching.hip, each tried on a scratch copy and not kept; "old" are the stereo tests that existed
before (test_matching_parity's test_stereo_rectified_*, test_resident_frame, test_tracker_vision):
  1 `cb += 32` -> one pass             every test of this file but the extractor's; old: all of them
  2 lex_less -> `dd < bestDist`        host entry (both sizes) and batch of 17, at frame tie_order only: the row's list is
                                       in index order unless a key reaches the row late in its band; old: none
  3 `endu >= lvw` -> `>`               host entry (both sizes), batch of 17 (frame refine); old: none
  4 the spill loop removed             host entry (both sizes), batches of 16 and 17 (frames big, big_reject); old: none
  5 `k = n / 2` -> `(n - 1) / 2`       host entry (both sizes), batches of 16 and 17 (first at frames rows, median_n2); old: host_api[1000]
                                       and test_resident_frame (both seeds), not host_api[1001], [1002], edge_cases, batch_device
  6 `rs[H]` from thread 0 in <256>     NOT caught, by nothing old or new, and no test inside the domain can: row_start[H]
                                       closes the list of the last image row, and a left key there has its patch outside
                                       the plane at every octave.  The batches of 17 run that kernel and
                                       would catch a wrong row_start[y] for any y <= h - 6 (fault 1 shows the lists are read)
  7 `octR > levelL + 1` -> `> levelL`  host entry (both sizes), batch of 17 (first at frame rows: right octave 1, left 0); old: all of them
  8 k_knn2: merge of wavefronts 1..3   test_matching_parity::test_knn2_popcount_kernel only (no other test runs k_knn2)
     dropped

Measured on an MI355X: this file 3.2 s for its 9 tests (2.3 s of it the two host-entry tests, mostly the oracle's answers for
the 44 planted frames); test_tall_frame_batch_entry, 34 images of 640 x 1030, 0.01 s after the shared frame is built.
"""
import numpy as np
import pytest

from tests import stereo_cases
from tests.oracle_lib import KEYPOINT_DTYPE
from vieo_slam_amd import synth
from vieo_slam_amd._lib import DeviceBuffer, VieoError, check, lib

pytestmark = pytest.mark.gpu
BF, BASELINE = stereo_cases.BF, stereo_cases.BASELINE
GUARD = np.uint32(0xDEADBEEF)
CAPACITY = 4352  # rows per image of the planted key arrays: the largest frame has 4148 left keys


def _hip(nfeat=300):
    from vieo_slam_amd.orb_extractor import ORBextractor
    return ORBextractor(nfeat, 1.2, 8, 20, 7)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Planted:
    """a frame, the oracle extractors that hold its pyramids and the oracle's answer"""

    def __init__(self, oracle, frame, ext=None):
        self.frame = frame
        if ext is None:
            ext = oracle.extractor(300), oracle.extractor(300)
            ext[0](frame.left), ext[1](frame.right)
        self.ext = ext
        self.ur, self.dp = oracle.stereo_match(ext[0], ext[1], frame.kl, frame.dl, frame.kr, frame.dr, BASELINE, BF)

    def cut(self, oracle, n_l, n_r):
        """the same images with the first n_l left and n_r right keys"""
        import copy
        f = copy.copy(self.frame)
        f.name = "%s[:%d,:%d]" % (f.name, n_l, n_r)
        f.kl, f.dl, f.kr, f.dr = f.kl[:n_l], f.dl[:n_l], f.kr[:n_r], f.dr[:n_r]
        return Planted(oracle, f, self.ext)


_cache = {}


def planted_frames(oracle, w, h):
    if (w, h) not in _cache:
        _cache[(w, h)] = [Planted(oracle, f) for f in stereo_cases.all_frames(w, h)]
    return _cache[(w, h)]


def planted_tall(oracle):
    if "tall" not in _cache:
        _cache["tall"] = Planted(oracle, stereo_cases.frame_tall(640, 1030))
    return _cache["tall"]


def host_entry(p, handles=None):
    from vieo_slam_amd.matching import compute_stereo_matches
    f = p.frame
    hL, hR = handles or (_hip(), _hip())
    hL(f.left), hR(f.right)
    return compute_stereo_matches(hL, hR, f.kl, f.dl, f.kr, f.dr, BASELINE, BF)


def batch_entry(ps, w, h, capacity=CAPACITY, repeat=1):
    """the frames of `ps` as one vieo_stereo_match_rectified_batch_device call on planted key arrays; the outputs are
    filled with a guard pattern first.  returns [(uright, depth) as uint32 [F, capacity]] per repetition"""
    F = len(ps)
    imgs = np.zeros((F, 2, h, w), np.uint8)
    K = np.zeros((2 * F, capacity), KEYPOINT_DTYPE)
    D = np.zeros((2 * F, capacity, 32), np.uint8)
    C = np.zeros((2 * F, 2), np.int32)
    for i, p in enumerate(ps):
        f = p.frame
        imgs[i, 0], imgs[i, 1] = f.left, f.right
        for side, (k, d) in enumerate(((f.kl, f.dl), (f.kr, f.dr))):
            assert len(k) <= capacity
            K[2 * i + side, :len(k)], D[2 * i + side, :len(k)], C[2 * i + side, 0] = k, d, len(k)
    hx = _hip()
    xcap = hx.max_keypoints()
    bufs = [DeviceBuffer(n) for n in (imgs.nbytes, 2 * F * xcap * 28, 2 * F * xcap * 32, 2 * F * 8, K.nbytes, D.nbytes, C.nbytes,
                                      F * capacity * 4, F * capacity * 4)]
    d_img, x_kp, x_desc, x_cnt, d_kp, d_desc, d_cnt, d_ur, d_dp = bufs
    d_img.upload(imgs)
    # the handle's pyramids: an extraction of the 2 F images (its own keys are not used)
    hx.extract_batch_device(d_img.ptr, 2 * F, w, h, w, w * h, x_kp.ptr, x_desc.ptr, xcap, x_cnt.ptr)
    hx.sync()
    d_kp.upload(K), d_desc.upload(D), d_cnt.upload(C)
    out = []
    for _ in range(repeat):
        guard = np.full((F, capacity), GUARD, np.uint32)
        d_ur.upload(guard), d_dp.upload(guard)
        check(lib().vieo_stereo_match_rectified_batch_device(hx._h, F, d_kp.ptr, d_desc.ptr, d_cnt.ptr, capacity, BASELINE, BF,
                                                             d_ur.ptr, d_dp.ptr), "vieo_stereo_match_rectified_batch_device")
        hx.sync()
        out.append((d_ur.download(np.uint32, (F, capacity)), d_dp.download(np.uint32, (F, capacity))))
    for b in bufs:
        b.free()
    return out


def assert_batch(ps, ur, dp):
    for i, p in enumerate(ps):
        n = len(p.frame.kl)
        assert np.array_equal(ur[i, :n], _bits(p.ur)), (i, p.frame.name)
        assert np.array_equal(dp[i, :n], _bits(p.dp)), (i, p.frame.name)
        assert (ur[i, n:] == GUARD).all() and (dp[i, n:] == GUARD).all(), (i, p.frame.name, "rows beyond the count were written")


@pytest.mark.parametrize("w,h", [(239, 239), (244, 241)])
def test_host_entry_planted_frames(oracle, w, h):
    handles = _hip(), _hip()
    for p in planted_frames(oracle, w, h):
        ur, dp = host_entry(p, handles)
        assert np.array_equal(_bits(ur), _bits(p.ur)), p.frame.name
        assert np.array_equal(_bits(dp), _bits(p.dp)), p.frame.name


def batch_of(oracle, n):
    """17: the first 17 planted frames; 16: the five special ones and the last eleven -- together all of them.  Both hold a
    frame without left keys, one without right keys, the two with more than 2048 left keys and the one with 65
    candidates in a row."""
    ps = planted_frames(oracle, 244, 241)
    assert len(ps) == 22
    ps = ps[:17] if n == 17 else ps[:5] + ps[-11:]
    names = [p.frame.name for p in ps]
    assert len(ps) == n and all(s in names for s in ("empty_left", "no_right", "big", "big_reject", "counts"))
    assert len({len(p.frame.kl) for p in ps}) > 8
    return ps


@pytest.mark.parametrize("n", [16, 17])
def test_batch_entry_planted_frames(oracle, n):
    """16 frames: k_stereo_rows<1024>, 17: k_stereo_rows<256>"""
    ps = batch_of(oracle, n)
    runs = batch_entry(ps, 244, 241, repeat=2 if n == 17 else 1)
    assert_batch(ps, *runs[0])
    handles = _hip(), _hip()
    for i, p in enumerate(ps):  # and the same frame alone through the host entry
        ur, dp = host_entry(p, handles)
        m = len(ur)
        assert np.array_equal(_bits(ur), runs[0][0][i, :m]) and np.array_equal(_bits(dp), runs[0][1][i, :m]), p.frame.name
    if n == 17:  # the same bytes again
        assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


def test_tall_frame_host_entry(oracle):
    """640 x 1030: more than 1024 rows, two rows a thread in the prefix sum of k_stereo_rows<1024>"""
    p = planted_tall(oracle)
    ur, dp = host_entry(p)
    assert np.array_equal(_bits(ur), _bits(p.ur)) and np.array_equal(_bits(dp), _bits(p.dp))
    assert (p.ur >= 0).sum() >= 6


def test_tall_frame_batch_entry(oracle):
    """the tall frame last in a batch of 17 of its size (k_stereo_rows<256>, five rows a thread); the other sixteen are
    the same images with fewer keys"""
    p = planted_tall(oracle)
    n_l, n_r = len(p.frame.kl), len(p.frame.kr)
    ps = [p.cut(oracle, (i * n_l) // 16, n_r - (i % 3)) for i in range(16)] + [p]
    ur, dp = batch_entry(ps, 640, 1030, capacity=64)[0]
    assert_batch(ps, ur, dp)


@pytest.mark.parametrize("n", [2, 16])
def test_tall_frame_small_batches(oracle, n):
    """k_stereo_rows<1024> on a batch of tall frames"""
    p = planted_tall(oracle)
    ps = [p.cut(oracle, len(p.frame.kl) - 1 - i % 4, len(p.frame.kr) - i % 5) for i in range(n - 1)] + [p]
    ur, dp = batch_entry(ps, 640, 1030, capacity=64)[0]
    assert_batch(ps, ur, dp)


def test_extractor_refuses_too_tall_then_extracts(oracle):
    """260 x 600 and 560 x 1030 have a level with round(regionW / regionH) == 0: the library refuses them, and the same
    handle then extracts 640 x 1030 equal to the oracle"""
    h = _hip()
    for w, hh in ((260, 600), (560, 1030)):
        with pytest.raises(VieoError, match="too tall"):
            h(synth.synth_image(5, w, hh))
    img = synth.synth_image(5, 640, 1030)
    mono, kps, desc = h(img)
    omono, okps, odesc = oracle.extractor(300)(img)
    assert mono == omono and len(kps) == len(okps) > 200
    assert np.array_equal(kps.view(np.uint8), okps.view(np.uint8)) and np.array_equal(desc, odesc)
