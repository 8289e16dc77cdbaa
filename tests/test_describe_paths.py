"""GPU parity tests of k_describe_fused's paths: the border (REFLECT_101) staging with one key point per wavefront, four
key points per wavefront in a batch whose images run out of key points at different places, and a level 0 that takes
the border staging for every key point while the pyramid levels take the dword one -- key points and descriptors bit
for bit against the CPU oracle's extractor.

The shapes are the smallest the planner accepts (tests/test_fast_cells.py: at least 239 pixels each way at eight levels
of 1.2; a device batch needs a dword-aligned stride, so 244 x 241 there).  A patch is staged with dword loads when it
lies inside its level (the key point at least 21 pixels from every side, the plane dword-aligned) and byte by byte
otherwise; key points exist from 16 pixels off the border, and the top levels of these images are 66 to 100 pixels wide.
"""
import numpy as np
import pytest

from vieo_slam_amd import synth
from vieo_slam_amd._lib import DeviceBuffer

from .test_orb_parity import _assert_same, _hip

pytestmark = pytest.mark.gpu
NFEAT = 300
RAW = 21  # radius of the raw patch (18 of the steered pattern + 3 of the blur)


def _border_keys(o, kps):
    """Key points of an oracle result whose 43 x 43 raw patch leaves their level, per level."""
    n = np.zeros(8, int)
    for l in range(8):
        w, h = o.level_size(l)
        k = kps[kps["octave"] == l]
        s = np.float32(o.scale_factors()[l])
        x, y = np.rint(k["x"] / s).astype(int), np.rint(k["y"] / s).astype(int)
        n[l] = np.count_nonzero((x < RAW) | (y < RAW) | (x + RAW >= w) | (y + RAW >= h))
    return n


def test_border_path_one_key_per_wavefront(oracle):
    img = synth.synth_image(2004, 239, 239)
    o = oracle.extractor(NFEAT)
    ref = o(img)
    per_level = np.bincount(ref[1]["octave"], minlength=8)
    assert per_level.min() > 0, per_level  # every level is present
    border = _border_keys(o, ref[1])
    assert border.sum() > 30 and np.count_nonzero(border) == 8, border  # and has key points on the border path
    assert border.sum() < len(ref[1])                                   # beside interior ones
    _assert_same(ref, _hip(NFEAT)(img))


def _batch_images():
    """32 images of 244 x 241 with different textures: one blank, one whose texture is a 60-pixel window."""
    B, w, h = 32, 244, 241
    imgs = np.stack([synth.synth_image(2100 + i, w, h) for i in range(B)])
    imgs[5] = 93
    few = np.full((h, w), 120, np.uint8)
    few[90:150, 100:160] = imgs[11][90:150, 100:160]
    imgs[11] = few
    return imgs


def test_four_keys_per_wavefront_ragged_batch(oracle):
    from vieo_slam_amd.orb_extractor import KEYPOINT_DTYPE
    imgs = _batch_images()
    B, hgt, w = imgs.shape
    o = oracle.extractor(NFEAT)
    refs = [o(im) for im in imgs]
    counts = np.array([len(r[1]) for r in refs])
    # the blank image has no record at all, the windowed one a handful, and the wavefronts' runs of four end inside a
    # run (a count that is no multiple of 4, let alone 16) at different places in different images
    assert counts[5] == 0 and 0 < counts[11] < 40, counts
    assert np.count_nonzero(counts % 16) > 0 and np.count_nonzero(counts % 4) > 0, counts
    assert len(set(counts.tolist())) > 8, counts
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
    assert np.array_equal(cnt[:, 0], counts)
    for i in range(B):
        n = cnt[i, 0]
        _assert_same(refs[i], (int(cnt[i, 1]), kps[i, :n], desc[i, :n]))


def test_unaligned_level0_border_staging_beside_dword_staging(oracle):
    # the view's base is not dword-aligned and its stride no multiple of 4: every level-0 patch is staged byte by byte,
    # the pyramid levels' interior patches with dwords, in one launch
    big = synth.synth_image(2020, 263, 250)
    view = big[3:244, 5:246]
    assert view.shape == (241, 241) and view.strides[0] % 4 and view.ctypes.data % 4
    o = oracle.extractor(NFEAT)
    ref = o(np.ascontiguousarray(view))
    per_level = np.bincount(ref[1]["octave"], minlength=8)
    border = _border_keys(o, ref[1])
    assert per_level[0] > border[0] and per_level[0] > 20, (per_level, border)  # level-0 keys that only the alignment sends to the border path
    assert (per_level[1:] - border[1:]).sum() > 50, (per_level, border)       # interior keys on the other levels
    _assert_same(ref, _hip(NFEAT)(view))
