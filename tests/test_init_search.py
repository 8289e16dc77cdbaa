"""ORBmatcher::SearchForInitialization on the device (vieo_search_for_initialization, csrc/init_search.hip) against the
restatement tests/mono_init_ref.py, which tests/test_init_search_ref.py holds against a brute-force statement: vnMatches12,
nmatches and vbPrevMatched bit for bit, and the candidate lists of the device stage through the tap."""
import numpy as np
import pytest

from tests import mono_init_ref as ref
from vieo_slam_amd import initialization as ini
from vieo_slam_amd.orb_extractor import KEYPOINT_DTYPE

pytestmark = pytest.mark.gpu

# frames of 0, 1, 65 and 300 keys: (seed, n1, n2, window)
SHAPES = [(11, 0, 0, 100), (12, 0, 65, 100), (13, 65, 0, 100), (14, 1, 1, 100), (15, 65, 65, 100), (16, 300, 300, 100),
          (17, 65, 300, 30), (18, 300, 65, 200), (19, 1, 300, 1000)]


def _want(pair, bounds, **kw):
    F1, F2, prev, window = pair
    return ref.search_for_initialization(F1.keys, F1.desc, F2.keys, F2.desc, prev, window, bounds, **kw)


def _same(got, want, prev_in):
    m12, n, prev = got
    assert np.array_equal(m12, want["matches12"])
    assert n == want["nmatches"]
    assert np.array_equal(prev.view(np.uint32), want["prev_matched"].view(np.uint32))
    assert prev is not prev_in


@pytest.fixture(scope="module")
def batch():
    pairs, bounds = [], None
    for seed, n1, n2, window in SHAPES:
        # (the large pair: wide families, so that distances fill the range up to the cut and ratio tests fail)
        kw = dict(n_families=4, max_flips=40) if n1 == n2 == 300 else {}
        F1, F2, prev, bounds = ini.make_search_pair(seed, n1, n2, dup=0.3, **kw)
        pairs.append((F1, F2, prev, window))
    return pairs, bounds, [_want(p, bounds) for p in pairs]


def test_a_batch_of_every_shape_equals_the_restatement(batch):
    pairs, bounds, want = batch
    got = ini.SearchForInitialization(pairs, bounds)
    for p, (g, w) in enumerate(zip(got, want)):
        _same(g, w, pairs[p][2])
        assert ini.search_for_initialization_tap(len(pairs[p][0].keys), p) == w["lists"], p
    assert sum(w["nmatches"] for w in want) > 100
    for k in ("steal", "skip_equal", "erased", "ratio_fail", "empty", "octave"):
        assert sum(w["stats"][k] for w in want) > 0, k
    assert any(d > ref.TH_LOW for w in want for lst in w["lists"] for _, d, _ in lst)  # entries in (TH_LOW, cut]
    # run to run
    again = ini.SearchForInitialization(pairs, bounds)
    for g, a in zip(got, again):
        assert np.array_equal(g[0], a[0]) and g[1] == a[1] and np.array_equal(g[2], a[2])


def test_a_pair_alone_and_in_any_split_gives_the_same(batch):
    pairs, bounds, want = batch
    for lo, hi in ((5, 6), (0, 4), (4, 9)):
        got = ini.SearchForInitialization(pairs[lo:hi], bounds)
        for p in range(lo, hi):
            _same(got[p - lo], want[p], pairs[p][2])
            assert ini.search_for_initialization_tap(len(pairs[p][0].keys), p - lo) == want[p]["lists"]
    assert ini.SearchForInitialization([], bounds) == []


def test_a_pool_that_is_too_small_is_grown_and_no_list_is_cut(batch, monkeypatch):
    pairs, bounds, want = batch
    listed = sum(len(lst) for lst in want[5]["lists"])
    assert listed > 64
    monkeypatch.setenv("VIEO_INIT_POOL", "7")
    got = ini.SearchForInitialization(pairs[5:7], bounds)
    for p in (5, 6):
        _same(got[p - 5], want[p], pairs[p][2])
        assert ini.search_for_initialization_tap(len(pairs[p][0].keys), p - 5) == want[p]["lists"]


@pytest.mark.parametrize("nn_ratio,check_orientation", [(0.75, True), (0.9, False), (0.6, True)])
def test_other_ratios_and_no_orientation_check(batch, nn_ratio, check_orientation):
    pairs, bounds, _ = batch
    sel = [pairs[4], pairs[5]]
    got = ini.SearchForInitialization(sel, bounds, nn_ratio, check_orientation)
    for k, g in enumerate(got):
        w = _want(sel[k], bounds, nn_ratio=nn_ratio, check_orientation=check_orientation)
        _same(g, w, sel[k][2])
        assert ini.search_for_initialization_tap(len(sel[k][0].keys), k) == w["lists"]  # the cut follows the ratio


def _key(x, y, angle=0.0, octave=0):
    k = np.zeros(1, KEYPOINT_DTYPE)
    k["x"], k["y"], k["angle"], k["octave"], k["size"], k["class_id"] = x, y, angle, octave, 31, -1
    return k


def _bits(*which):
    d = np.zeros(32, np.uint8)
    for b in which:
        d[b >> 3] |= 1 << (b & 7)
    return d


def test_planted_steal_equal_distance_skip_and_histogram_erasure():
    rng = np.random.default_rng(21)
    bounds = np.array([0, 752, 0, 480], np.float32)
    # second frame: A (all zero), B, an octave-1 twin of A nearer than A, and 12 keys apart from one another
    k2 = [_key(100, 100), _key(300, 100), _key(100.5, 100, octave=1)]
    d2 = [_bits(), rng.integers(0, 256, 32, dtype=np.uint8), _bits()]
    # first frame: 0 takes A at 10 bits; 1 steals it at 5; 2 meets it at 5 again, the equal-distance skip, and has nothing
    # else; 3 takes B alone in its rotation bin, 1 of 15 matches: erased; 4 sits above octave 0
    k1 = [_key(100, 100, 20), _key(102, 100, 20), _key(101, 101, 20), _key(300, 100, 200), _key(100, 100, 20, octave=2)]
    d1 = [_bits(*range(10)), _bits(*range(5)), _bits(*range(100, 105)), d2[1].copy(), _bits()]
    for k in range(12):
        k2.append(_key(50 + 40 * k, 300))
        d2.append(rng.integers(0, 256, 32, dtype=np.uint8))
        k1.append(_key(51 + 40 * k, 301, 20))
        d1.append(d2[-1].copy())
    F1, F2 = ini.InitFrame(np.concatenate(k1), np.stack(d1)), ini.InitFrame(np.concatenate(k2), np.stack(d2))
    prev = np.stack([F1.keys["x"], F1.keys["y"]], axis=1)
    want = _want((F1, F2, prev, 10), bounds)
    s = want["stats"]
    assert (s["steal"], s["skip_equal"], s["erased"], s["octave"]) == (1, 1, 1, 1)
    assert list(want["matches12"][:5]) == [-1, 0, -1, -1, -1] and want["nmatches"] == 13
    got = ini.SearchForInitialization([(F1, F2, prev, 10)], bounds)[0]
    _same(got, want, prev)
    assert ini.search_for_initialization_tap(len(F1.keys), 0) == want["lists"]
    # the stolen key keeps its own position, the thief gets A's
    assert tuple(got[2][0]) == (100.0, 100.0) and tuple(got[2][1]) == (100.0, 100.0) and tuple(got[2][2]) == (101.0, 101.0)


def test_windows_clipped_at_each_border_and_outside_the_image():
    rng = np.random.default_rng(22)
    bounds = np.array([0, 752, 0, 480], np.float32)
    n2 = 300
    k2 = np.zeros(n2, KEYPOINT_DTYPE)
    # keys crowded along the four borders, the last cells' rounding edge included
    side = rng.integers(0, 4, n2)
    along, depth = rng.uniform(0, 1, n2), rng.uniform(0, 30, n2)
    k2["x"] = np.choose(side, [depth, 752 - depth, along * 752, along * 752])
    k2["y"] = np.choose(side, [along * 480, along * 480, depth, 480 - depth])
    k2["size"], k2["class_id"] = 31, -1
    d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    pick = rng.permutation(n2)[:65]
    k1 = k2[pick].copy()
    F1, F2 = ini.InitFrame(k1, d2[pick]), ini.InitFrame(k2, d2)
    prev = np.stack([k1["x"], k1["y"]], axis=1).astype(np.float32)
    # windows centred up to 60 pixels outside each border: clipped, or empty
    prev += rng.uniform(-1, 1, prev.shape).astype(np.float32) * np.float32(60)
    prev[:4] = [[-500, 100], [2000, 100], [100, -500], [100, 2000]]
    want = _want((F1, F2, prev, 50), bounds)
    assert want["stats"]["empty"] >= 4 and want["nmatches"] > 20
    assert any(ref.pos_in_grid(x, y, bounds) is None for x, y in zip(k2["x"], k2["y"]))  # keys that are in no cell
    # a second pair in the same call: 200 keys in ONE column of cells, whose run a wavefront walks in four steps; near
    # descriptors, so that the lists are long and their order shows
    kc = np.zeros(200, KEYPOINT_DTYPE)
    kc["x"], kc["y"], kc["size"], kc["class_id"] = rng.uniform(0, 3, 200), rng.uniform(0, 470, 200), 31, -1
    dc = np.zeros((200, 32), np.uint8)
    dc[:, :8] = rng.integers(0, 256, (200, 8), dtype=np.uint8)
    Fc1, Fc2 = ini.InitFrame(kc[:9], dc[:9]), ini.InitFrame(kc, dc)
    prev_c = np.stack([kc["x"][:9], kc["y"][:9]], axis=1).astype(np.float32)
    want_c = _want((Fc1, Fc2, prev_c, 1000), bounds)
    assert max(len(lst) for lst in want_c["lists"]) > 128 and max(o for lst in want_c["lists"] for _, _, o in lst) >= 192
    got = ini.SearchForInitialization([(F1, F2, prev, 50), (Fc1, Fc2, prev_c, 1000)], bounds)
    _same(got[0], want, prev)
    _same(got[1], want_c, prev_c)
    assert ini.search_for_initialization_tap(len(F1.keys), 0) == want["lists"]
    assert ini.search_for_initialization_tap(len(Fc1.keys), 1) == want_c["lists"]
