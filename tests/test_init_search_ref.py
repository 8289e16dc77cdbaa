"""The restatement of ORBmatcher::SearchForInitialization (tests/mono_init_ref.py) against its second, brute-force statement on
random tables that reach every branch of the walk, and the bound on the candidates the device hands back -- before the GPU
tests use the restatement as their yardstick (no GPU)."""
import numpy as np
import pytest

from tests import mono_init_ref as ref
from vieo_slam_amd import initialization as ini

# (seed, n1, n2, window): a dense one with many duplicates, a sparse one, one with a small window, a wide family
TABLES = [(1, 220, 160, 100, dict(dup=0.3)), (2, 150, 300, 40, dict()), (3, 200, 120, 15, dict(dup=0.4, shift=6.0)),
          (4, 180, 180, 100, dict(n_families=4, max_flips=40, dup=0.25))]


@pytest.fixture(scope="module")
def runs():
    out = []
    for seed, n1, n2, window, kw in TABLES:
        F1, F2, prev, bounds = ini.make_search_pair(seed, n1, n2, **kw)
        out.append((F1, F2, prev, bounds, window, ref.search_for_initialization(F1.keys, F1.desc, F2.keys, F2.desc, prev, window, bounds)))
    return out


def test_the_walk_equals_the_brute_force_statement(runs):
    for F1, F2, prev, bounds, window, r in runs:
        m, n, p = ref.search_for_initialization_brute(F1.keys, F1.desc, F2.keys, F2.desc, prev, window, bounds)
        assert np.array_equal(m, r["matches12"]) and n == r["nmatches"] == int((r["matches12"] >= 0).sum())
        assert np.array_equal(p.view(np.uint32), r["prev_matched"].view(np.uint32))
        # vbPrevMatched: the matched key's position where a match survives, untouched elsewhere
        hit = r["matches12"] >= 0
        assert np.array_equal(r["prev_matched"][~hit], prev[~hit]) and n > 0


def test_without_the_orientation_check_too(runs):
    F1, F2, prev, bounds, window, r = runs[0]
    a = ref.search_for_initialization(F1.keys, F1.desc, F2.keys, F2.desc, prev, window, bounds, check_orientation=False)
    m, n, p = ref.search_for_initialization_brute(F1.keys, F1.desc, F2.keys, F2.desc, prev, window, bounds, check_orientation=False)
    assert np.array_equal(m, a["matches12"]) and n == a["nmatches"] and a["stats"]["erased"] == 0
    assert a["nmatches"] == r["nmatches"] + r["stats"]["erased"]


def test_the_tables_reach_every_branch(runs):
    total = {}
    for *_, r in runs:
        for k, v in r["stats"].items():
            total[k] = total.get(k, 0) + v
    # the steal, the equal-distance skip (and the smaller-distance one), the empty window, an octave above 0, the histogram
    # erasure, a failed ratio test, a best beyond TH_LOW, an accepted match whose second best lies in (TH_LOW, cut]
    for k in ("steal", "skip_equal", "skip_less", "empty", "octave", "erased", "ratio_fail", "over_low"):
        assert total[k] > 0, (k, total)


def test_the_bound_on_the_listed_candidates():
    # 0.9: 55 * 0.9f <= 50 < 56 * 0.9f, in float as :677 computes it
    assert ref.list_cut(0.9) == 55
    assert ref.f32(55) * ref.f32(0.9) <= ref.f32(50) < ref.f32(56) * ref.f32(0.9)
    assert ref.list_cut(1.0) == 50 and ref.list_cut(2.0) == 50 and ref.list_cut(0.5) == 100 and ref.list_cut(0.1) == 256
    # the decision of :676-677 for every (bestDist, bestDist2): a second best beyond the cut decides as INT_MAX does
    for nn in (0.9, 0.75, 0.6):
        cut = ref.list_cut(nn)
        for best in range(0, ref.TH_LOW + 1):
            for second in range(cut + 1, 257):
                assert ref.f32(best) < ref.f32(second) * ref.f32(nn)


def test_the_walk_over_the_lists_alone_gives_the_same_matches(runs):
    """what the library's host half does: the walk over the candidates with distance <= cut only"""
    for F1, F2, prev, bounds, window, r in runs:
        n2 = len(F2.keys)
        dist, m21, m12, hist = [ref.INT_MAX] * n2, [-1] * n2, np.full(len(F1.keys), -1, np.int32), [[] for _ in range(30)]
        for i1, lst in enumerate(r["lists"]):
            best, best2, idx = ref.INT_MAX, ref.INT_MAX, -1
            for key, d, _ in lst:
                if dist[key] <= d:
                    continue
                if d < best:
                    best2, best, idx = best, d, key
                elif d < best2:
                    best2 = d
            if best <= ref.TH_LOW and ref.f32(best) < ref.f32(best2) * ref.f32(0.9):
                if m21[idx] >= 0:
                    m12[m21[idx]] = -1
                m12[i1], m21[idx], dist[idx] = idx, i1, best
                hist[ref.rot_bin(F1.keys["angle"][i1], F2.keys["angle"][idx])].append(i1)
        keep = ref.compute_three_maxima([len(h) for h in hist])
        for b in range(30):
            if b not in keep:
                m12[hist[b]] = -1
        assert np.array_equal(m12, r["matches12"])
    # the lists do hold entries in (TH_LOW, cut]
    assert any(d > ref.TH_LOW for *_, r in runs for lst in r["lists"] for _, d, _ in lst)


def test_grid_edges():
    b = np.array([0, 752, 0, 480], np.float32)
    # a key on the right or lower border rounds into cell 64 / 48: in no cell (PosInGrid)
    assert ref.pos_in_grid(751.9, 10, b) is None and ref.pos_in_grid(10, 479.9, b) is None and ref.pos_in_grid(-10, 5, b) is None
    assert ref.pos_in_grid(0, 0, b) == (0, 0) and ref.pos_in_grid(745, 474, b) == (63, 47)
    # windows clipped at each border, and windows wholly outside
    assert ref.cell_range(5, 5, 100, b)[0::2] == (0, 0) and ref.cell_range(750, 478, 100, b)[1::2] == (63, 47)
    assert ref.cell_range(900, 100, 100, b) is None and ref.cell_range(100, 700, 100, b) is None
    assert ref.cell_range(-200, 100, 100, b) is None and ref.cell_range(100, -200, 100, b) is None
    assert ref.c_round(0.5) == 1 and ref.c_round(1.5) == 2 and ref.c_round(2.5) == 3 and ref.c_round(-0.5) == -1
