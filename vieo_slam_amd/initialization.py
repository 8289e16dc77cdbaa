"""Monocular initialisation, the matcher: ORBmatcher::SearchForInitialization (reference src/ORBmatcher.cc:628-723) for a
batch of frame pairs in one call of vieo_search_for_initialization (csrc/init_search.hip) -- the first step of
Tracking::MonocularInitialization of every sequence that is initialising.  The device lists, per octave-0 key of a first
frame, the window candidates that can change an outcome; the order-dependent walk, the rotation histogram and vbPrevMatched
are replayed on the host inside the library.  There is no CPU path here: without a gfx950 device the call raises."""
import numpy as np

from . import _lib
from .orb_extractor import KEYPOINT_DTYPE

TH_LOW = 50
NN_RATIO_INIT, WINDOW_INIT = 0.9, 100  # ORBmatcher matcher(0.9, true); matcher.SearchForInitialization(..., 100) (Tracking.cc:1519-1520)

INIT_PAIR_DTYPE = np.dtype([("keys1", "<u8"), ("desc1", "<u8"), ("keys2", "<u8"), ("desc2", "<u8"), ("prev_matched", "<u8"),
                            ("matches12", "<u8"), ("n1", "<i4"), ("n2", "<i4"), ("window_size", "<i4"), ("n_matches", "<i4")])
assert INIT_PAIR_DTYPE.itemsize == 64


class InitFrame:
    """what the matcher reads of a Frame: mvKeysUn and mDescriptors"""

    def __init__(self, keys, descriptors):
        self.keys = np.ascontiguousarray(keys, KEYPOINT_DTYPE).reshape(-1)
        self.desc = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
        if len(self.keys) != len(self.desc):
            raise ValueError("%d keys, %d descriptor rows" % (len(self.keys), len(self.desc)))


def _ptr(a):
    return a.ctypes.data if a.size else 0


def search_for_initialization_call(pairs, bounds, nn_ratio=NN_RATIO_INIT, check_orientation=True):
    """vieo_search_for_initialization, raw: pairs = [(F1, F2, prev_matched [n1, 2], window_size)] with F1 / F2 InitFrame;
    returns (rc, [(matches12, nmatches, prev_matched after the call)])"""
    recs = np.zeros(len(pairs), INIT_PAIR_DTYPE)
    out = []
    for p, (F1, F2, prev, window) in enumerate(pairs):
        prev = np.array(prev, np.float32).reshape(-1, 2)
        if len(prev) != len(F1.keys):
            raise ValueError("pair %d: %d keys, %d entries of prev_matched" % (p, len(F1.keys), len(prev)))
        m12 = np.full(len(F1.keys), -7, np.int32)  # (a refused call leaves it)
        out.append((m12, prev))
        r = recs[p]
        r["keys1"], r["desc1"], r["keys2"], r["desc2"] = _ptr(F1.keys), _ptr(F1.desc), _ptr(F2.keys), _ptr(F2.desc)
        r["prev_matched"], r["matches12"] = _ptr(prev), _ptr(m12)
        r["n1"], r["n2"], r["window_size"], r["n_matches"] = len(F1.keys), len(F2.keys), int(window), -7
    b = np.ascontiguousarray(bounds, np.float32).reshape(4)
    rc = _lib.lib().vieo_search_for_initialization(recs.ctypes.data if len(recs) else None, len(recs), b.ctypes.data,
                                                   float(nn_ratio), int(bool(check_orientation)))
    return rc, [(m12, int(recs[p]["n_matches"]), prev) for p, (m12, prev) in enumerate(out)]


def SearchForInitialization(pairs, bounds, nn_ratio=NN_RATIO_INIT, check_orientation=True):
    """int ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) for every pair of the list in
    one call.  pairs: [(F1, F2, prev_matched [n1, 2] float32, window_size)]; bounds = (min x, max x, min y, max y) of the
    frames' grid.  returns [(vnMatches12, the return value, vbPrevMatched after the call)]; the caller's prev_matched is not
    written."""
    rc, out = search_for_initialization_call(pairs, bounds, nn_ratio, check_orientation)
    _lib.check(rc, "vieo_search_for_initialization")
    return out


def search_for_initialization_tap(n1, pair):
    """the device stage of pair `pair` of the last SearchForInitialization: per key of the first frame the [(key of the
    second frame, distance, position in the reference's walk over the window's cells)] of every listed candidate"""
    L = _lib.lib()
    cnt = np.zeros(max(n1, 1), np.int32)
    _lib.check(L.vieo_search_for_initialization_tap(pair, cnt.ctypes.data, None, None, None, 0), "vieo_search_for_initialization_tap")
    cap = max(int(cnt.max()), 1)
    key, dist, order = (np.zeros((len(cnt), cap), np.int32) for _ in range(3))
    _lib.check(L.vieo_search_for_initialization_tap(pair, None, key.ctypes.data, dist.ctypes.data, order.ctypes.data, cap),
               "vieo_search_for_initialization_tap")
    return [[(int(key[i, e]), int(dist[i, e]), int(order[i, e])) for e in range(cnt[i])] for i in range(n1)]


def make_search_pair(seed, n1, n2, width=752, height=480, n_families=None, dup=0.15, octave0=0.75, shift=12.0, far=0.05,
                     max_flips=14):
    """Two frames of synthetic keys for the matcher -> (F1, F2, prev_matched, bounds).  The second frame's descriptors come
    in families (a base row with up to max_flips bits flipped), so that windows hold near neighbours, equal distances
    and failed ratio tests.  Key i of the first frame restates a key of the second, moved by up to `shift` pixels with a few
    bits flipped and the angle turned by a common rotation; a share `dup` of them restate the SAME key as an earlier one
    (steals and the equal-distance skip), a share `far` sits near or beyond the image border (clipped and empty windows),
    one in ten carries an angle of its own (the histogram's losers).  prev_matched = the first frame's key positions, as
    Tracking::MonocularInitialization sets mvbPrevMatched."""
    rng = np.random.default_rng(seed)
    bounds = np.array([0, width, 0, height], np.float32)

    def flip(rows, most):
        rows = rows.copy()
        for r in rows:
            for bit in rng.integers(0, 256, rng.integers(0, most + 1)):
                r[bit >> 3] ^= 1 << (bit & 7)
        return rows

    n_fam = max(1, n_families if n_families is not None else (n2 + 1) // 2)
    base = rng.integers(0, 256, (n_fam, 32), dtype=np.uint8)
    k2 = np.zeros(n2, KEYPOINT_DTYPE)
    k2["x"], k2["y"] = rng.uniform(0, width, n2), rng.uniform(0, height, n2)
    k2["octave"] = np.where(rng.random(n2) < octave0, 0, rng.integers(1, 4, n2))
    k2["angle"] = rng.uniform(0, 360, n2).astype(np.float32) % np.float32(360)
    k2["size"], k2["class_id"] = 31, -1
    d2 = flip(base[rng.integers(0, n_fam, n2)], max_flips) if n2 else np.zeros((0, 32), np.uint8)
    k1 = np.zeros(n1, KEYPOINT_DTYPE)
    k1["size"], k1["class_id"] = 31, -1
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    k1["x"], k1["y"] = rng.uniform(0, width, n1), rng.uniform(0, height, n1)
    k1["angle"] = rng.uniform(0, 360, n1).astype(np.float32) % np.float32(360)
    k1["octave"] = np.where(rng.random(n1) < octave0, 0, rng.integers(1, 4, n1))
    src = np.full(n1, -1)
    for i in range(n1 if n2 else 0):
        src[i] = src[rng.integers(0, i)] if i and rng.random() < dup else rng.integers(0, n2)
        if src[i] < 0:
            continue
        j = src[i]
        k1["x"][i], k1["y"][i] = k2["x"][j] + rng.uniform(-shift, shift), k2["y"][j] + rng.uniform(-shift, shift)
        d1[i] = flip(d2[j:j + 1], 6)[0]
        if rng.random() < 0.9:
            k1["angle"][i] = np.float32((np.float64(k2["angle"][j]) + 20.0 + rng.uniform(-3, 3)) % 360.0) % np.float32(360)
    for i in np.nonzero(rng.random(n1) < far)[0]:
        side = rng.integers(0, 4)
        off = rng.uniform(-150, 5)
        k1["x"][i] = (off, width - off, k1["x"][i], k1["x"][i])[side]
        k1["y"][i] = (k1["y"][i], k1["y"][i], off, height - off)[side]
    prev = np.stack([k1["x"], k1["y"]], axis=1).astype(np.float32)
    return InitFrame(k1, d1), InitFrame(k2, d2), prev, bounds
