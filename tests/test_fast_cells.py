"""GPU parity tests of k_fast's per-cell set-up: the plan records, the division-free item index, the straight-line
tile staging and the branch-free pass C, bit for bit against the CPU oracle.

The shapes are the smallest the planner accepts (every level needs a 35-pixel cell region: at least 239 pixels each
way at eight levels of 1.2) whose cells reach the corners of the staging, enumerated with the planner's formulas:
241 x 241 has a cell 65 wide at an odd column (a 17th dword column) and 65 high (more than 64 rows), every ch % 4 and
every byte alignment; 239 x 251 has heights up to 69 and 64-wide cells of 16 dwords (the last column of the 16-lane
form); 239 x 247 has no cell height divisible by 4 (every last staging step overlaps its predecessor); 239 x 239 is
the smallest geometry there is (66 cells, the top level a single cell).
"""
import numpy as np
import pytest

from vieo_slam_amd import synth
from vieo_slam_amd._lib import DeviceBuffer

from .test_orb_parity import _assert_same, _hip

pytestmark = pytest.mark.gpu
NFEAT = 300


def _check(oracle, img, h=None, src=None):
    """tap_candidates(l) of every level, then keypoints and descriptors end to end; src = the (strided) view to extract."""
    o = oracle.extractor(NFEAT)
    h = h or _hip(NFEAT)
    ref = o(np.ascontiguousarray(img))
    got = h(img if src is None else src)
    for l in range(8):
        assert np.array_equal(h.tap_candidates(l), o.candidates(l)), "FAST level %d" % l
    _assert_same(ref, got)
    return ref, o


@pytest.mark.parametrize("seed,w,h", [(2001, 241, 241), (2002, 239, 251), (2003, 239, 247), (2004, 239, 239)])
def test_cell_shapes(oracle, seed, w, h):
    ref, _ = _check(oracle, synth.synth_image(seed, w, h))
    assert len(ref[1]) > 100


def test_low_contrast_second_round(oracle):
    # most cells find nothing at iniThFAST and take the second round at minThFAST
    img = (synth.synth_image_f32(2010, 239, 251) - 128.0) * 0.12 + 128.0
    ref, _ = _check(oracle, synth.quantise(img.astype(np.float32), 2010))
    assert len(ref[1]) > 100


def test_uniform_noise_dense_fallback(oracle):
    # the candidate list fills: pass B runs inside pass A and the dense fallback is taken
    img = np.random.default_rng(9).integers(0, 256, (241, 241), dtype=np.uint8)
    _, o = _check(oracle, img)
    assert len(o.candidates(0)) > 1000


def test_strided_unaligned_level0(oracle):
    # the stride is no multiple of 4 and the view's base is not dword-aligned
    big = synth.synth_image(2020, 263, 250)
    view = big[3:244, 5:246]
    assert view.shape == (241, 241) and view.strides[0] % 4 and view.ctypes.data % 4
    _check(oracle, view, src=view)


def test_batch_item_index(oracle):
    # 10 images x 71 cells = 710 items on a grid padded to 768: the division-free image / cell index (device images
    # need a dword-aligned stride: 244 x 241 is the 241 x 241 geometry's nearest neighbour with one)
    from vieo_slam_amd.orb_extractor import KEYPOINT_DTYPE
    B, w, hgt = 10, 244, 241
    imgs = np.stack([synth.synth_image(2030 + i, w, hgt) for i in range(B)])
    h = _hip(NFEAT)
    cap = h.max_keypoints()
    d_img = DeviceBuffer(imgs.nbytes)
    d_img.upload(imgs)
    d_kp, d_desc, d_cnt = DeviceBuffer(B * cap * 28), DeviceBuffer(B * cap * 32), DeviceBuffer(B * 8)
    h.extract_batch_device(d_img.ptr, B, w, hgt, w, w * hgt, d_kp.ptr, d_desc.ptr, cap, d_cnt.ptr)
    h.sync()
    cnt = d_cnt.download(np.int32, (B, 2))
    kps = d_kp.download(KEYPOINT_DTYPE, (B, cap))
    desc = d_desc.download(np.uint8, (B, cap, 32))
    o, single = oracle.extractor(NFEAT), _hip(NFEAT)
    for i in range(B):
        n = cnt[i, 0]
        got = (int(cnt[i, 1]), kps[i, :n], desc[i, :n])
        _assert_same(o(imgs[i]), got)
        _assert_same(single(imgs[i]), got)
