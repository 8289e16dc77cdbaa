"""Place recognition: the vocabulary, vieo_bow_transform and vieo_kfdb.

CPU tests certify the restatement of tests/bow_ref.py (hand-computed values, score identities, the literal inverted-file
database against the batched formulation, the file formats); GPU tests hold the library against that restatement."""
import ctypes

import numpy as np
import pytest

from tests import bow_ref as br
from vieo_slam_amd import _lib
from vieo_slam_amd import place_recognition as pr


def _desc(b0):
    d = np.zeros(32, np.uint8)
    d[0] = b0
    return d


def _table(rows):
    t = np.zeros(len(rows), pr.VOC_NODE_DTYPE)
    for i, (parent, leaf, b0, w) in enumerate(rows):
        t[i] = (parent, leaf, _desc(b0), w)
    return t


# node id: (parent, is_leaf, byte 0 of the descriptor (the other 31 are zero), weight)
HAND = _table([(0, 0, 0x00, 0.0),   # 1
               (1, 1, 0x01, 2.0),   # 2  word 0
               (1, 1, 0x06, 0.0),   # 3  word 1, stopped
               (0, 0, 0xF0, 0.0),   # 4
               (4, 1, 0xF1, 3.0),   # 5  word 2
               (4, 1, 0x70, 1.0)])  # 6  word 3
HAND_KEYS = np.stack([_desc(b) for b in (0x01, 0x03, 0x06, 0xF1, 0x30, 0x70)])


def test_hand_computed_vocabulary():
    """k = 2, L = 2: the root and six nodes, descriptors differing in byte 0 only (table above).  Keys, with the Hamming
    distances to (node 1, node 4) and then to the winner's two children:
      0x01: (1, 5) -> 1; (0, 3) -> node 2, word 0, weight 2
      0x03: (2, 6) -> 1; (1, 2) -> node 2, word 0
      0x06: (2, 6) -> 1; (3, 0) -> node 3, word 1, weight 0: stopped, in neither vector
      0xF1: (5, 1) -> 4; (0, 2) -> node 5, word 2, weight 3
      0x30: (2, 2) a TIE -> the first, node 1; (3, 4) -> node 2, word 0
      0x70: (3, 1) -> 4; (2, 0) -> node 6, word 3, weight 1
    v = {0: 2 + 2 + 2, 2: 3, 3: 1}, L1 norm 10 -> {0: 0.6, 2: 0.3, 3: 0.1}.
    levelsup = 1 (level 1): {1: [0, 1, 4], 4: [3, 5]}; levelsup = 0: {2: [0, 1, 4], 5: [3], 6: [5]}; levelsup = 2 and 3
    (L - levelsup <= 0): {0: [0, 1, 3, 4, 5]}."""
    voc = br.RefVocabulary(2, 2, HAND)
    assert voc.n_words == 4
    ids, vals, fv = voc.transform(HAND_KEYS, 1)
    assert ids.tolist() == [0, 2, 3]
    assert vals.tolist() == [6.0 / 10.0, 3.0 / 10.0, 1.0 / 10.0]
    assert abs(vals.sum() - 1.0) < 1e-15
    assert fv == [(1, [0, 1, 4]), (4, [3, 5])]
    assert voc.transform(HAND_KEYS, 0)[2] == [(2, [0, 1, 4]), (5, [3]), (6, [5])]
    for levelsup in (2, 3):  # levelsup >= L: the root
        assert voc.transform(HAND_KEYS, levelsup)[2] == [(0, [0, 1, 3, 4, 5])]
    assert voc.transform_one(HAND_KEYS[4], 1) == (0, 2.0, 1)  # the tie
    assert voc.transform_one(HAND_KEYS[2], 1) == (1, 0.0, 1)  # the stopped word
    assert voc.transform(HAND_KEYS[2:3], 1)[0].size == 0 and voc.transform(HAND_KEYS[2:3], 1)[2] == []


# a leaf at level 1 of an L = 2 tree: node 1 is a word already
EARLY = _table([(0, 1, 0x00, 1.5), (0, 0, 0xF0, 0.0), (2, 1, 0xF1, 1.0), (2, 1, 0x70, 1.0)])


def test_leaf_above_the_reported_level():
    """key 0x01 stops at node 1 (level 1).  levelsup = 0 asks for level 2, which the descent never reaches: the leaf's
    own id, 1, is reported (the reference leaves nid uninitialised); levelsup = 1 asks for level 1: node 1 as well;
    levelsup = 2: the root."""
    voc = br.RefVocabulary(2, 2, EARLY)
    assert voc.transform_one(_desc(0x01), 0) == (0, 1.5, 1)
    assert voc.transform_one(_desc(0x01), 1) == (0, 1.5, 1)
    assert voc.transform_one(_desc(0x01), 2) == (0, 1.5, 0)
    assert voc.transform_one(_desc(0xF1), 0) == (1, 1.0, 3)
    assert voc.transform_one(_desc(0xF1), 1) == (1, 1.0, 2)


def test_score_identities():
    rng = np.random.default_rng(5)
    n_voc = 500
    for _ in range(10):
        a = br.random_bow(rng, n_voc, int(rng.integers(5, 200)))
        b = br.random_bow(rng, n_voc, int(rng.integers(5, 200)), a, 0.5)
        assert abs(br.score(*a, *a) - 1.0) < 1e-14
        # symmetric: |v - w| is, and -|v| - |w| is up to the order of two subtractions; with <= 200 shared words and
        # sum |terms| <= 4 the two walks differ by at most 200 * 2^-53 * 4 = 9e-14
        assert abs(br.score(*a, *b) - br.score(*b, *a)) < 1e-13
        da, db = np.zeros(n_voc), np.zeros(n_voc)
        da[a[0]], db[b[0]] = a[1], b[1]
        assert abs(br.score(*a, *b) - (1.0 - 0.5 * np.abs(da - db).sum())) < 1e-13
        assert 0.0 < br.score(*a, *b) < 1.0
    lo = br.random_bow(rng, 100, 30)
    hi = (lo[0] + 100).astype(np.uint32), lo[1]
    assert br.score(*lo, *hi) == 0.0 and br.score(lo[0][:0], lo[1][:0], *lo) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
class _Library:
    """the library's KeyFrameDatabase under the scenario's calls"""

    def __init__(self, voc):
        self.db = pr.KeyFrameDatabase(voc)
        self.add, self.erase, self.set_covisible = self.db.add, self.db.erase, self.db.set_covisible
        self.detect_reloc, self.detect_loop, self.scores = self.db.detect_reloc, self.db.detect_loop, self.db.scores

    @property
    def tap(self):
        return self.db.tap_query()


def run_scenario(db, scene):
    """The calls of the database tests; returns the lists and taps in call order."""
    out = []
    for kf_id, ids, vals in scene["kfs"]:
        db.add(kf_id, ids, vals)
    for kf_id, c in scene["covis"].items():
        db.set_covisible(kf_id, c)
    all_ids = [k[0] for k in scene["kfs"]]
    (q0, q1), nothing = scene["queries"], scene["nothing"]
    out.append(("reloc q0", db.detect_reloc(*q0), db.tap))
    out.append(("scores q1", db.scores(*q1, all_ids[::3]), None))
    for kf_id in all_ids[2::5]:  # erases in the middle: covisible lists now name erased ids
        db.erase(kf_id)
    out.append(("reloc q1 after erases (stale scores of q0)", db.detect_reloc(*q1), db.tap))
    out.append(("reloc q0 again (stale scores of q1)", db.detect_reloc(*q0), db.tap))
    out.append(("reloc nothing shared", db.detect_reloc(*nothing), db.tap))
    out.append(("loop q0, min_score below every score", db.detect_loop(*q0, scene["connected"], 0.0), db.tap))
    out.append(("loop q1 (stale loop scores)", db.detect_loop(*q1, scene["connected"], 0.0), db.tap))
    out.append(("loop q0, min_score above every score", db.detect_loop(*q0, scene["connected"], 2.0), db.tap))
    out.append(("loop q1, nothing connected", db.detect_loop(*q1, [], 0.0), db.tap))
    if len(all_ids) > 2:  # an erased id comes back as a new key frame (scores 0, a new sequence number)
        db.add(all_ids[2], *q0)
        out.append(("reloc q1 after a re-add", db.detect_reloc(*q1), db.tap))
    return out


DB_SIZES = (0, 1, 70, 300)
DB_SEED = {0: 11, 1: 12, 70: 13, 300: 14}
DB_WORDS = 6000  # words of the vocabulary the GPU test builds are at least this many (asserted there)
_scene_cache, _ref_cache = {}, {}


def _scene(n):
    if n not in _scene_cache:
        _scene_cache[n] = br.make_database_scene(DB_SEED[n], n, DB_WORDS)
    return _scene_cache[n]


def _reference_run(n):
    if n not in _ref_cache:
        db = br.BatchedDatabase()
        _ref_cache[n] = (run_scenario(db, _scene(n)), list(db.margins))
    return _ref_cache[n]


class _LiteralWithTap(br.LiteralDatabase):
    tap = None

    def scores(self, ids, vals, kf_ids):
        return np.array([br.score(ids, vals, self.kfs[i].ids, self.kfs[i].vals) for i in kf_ids])


@pytest.mark.parametrize("n", DB_SIZES)
def test_literal_database_equals_batched(n):
    """the inverted file with stamps and the score-everything formulation return the same lists, order included: erases
    in the middle, consecutive queries reading stale scores, connected key frames for the loop form"""
    lit = run_scenario(_LiteralWithTap(), _scene(n))
    ref, _ = _reference_run(n)
    assert len(lit) == len(ref)
    n_lists = 0
    for (what, a, _), (_, b, _) in zip(lit, ref):
        if what.startswith("scores"):
            continue
        assert a == b, what
        n_lists += len(a)
    if n >= 70:
        assert n_lists > 8  # the scenario is not vacuous
        assert any(len(b) > 1 for w, b, _ in ref if not w.startswith("scores"))


@pytest.mark.parametrize("n", DB_SIZES)
def test_database_decisions_keep_their_margin(n):
    """no threshold decision of the restatement (0.75f * bestAccScore, minScore, the float compare of neighbour scores)
    lies within 1e-6 of its threshold for the seeds of the GPU test, so a rounding flip on the device cannot pass as, or
    hide as, a mismatch"""
    _, margins = _reference_run(n)
    assert all(m > 1e-6 for m in margins), min(margins)
    if n >= 70:
        assert len(margins) > 20


def test_vocabulary_files_round_trip(tmp_path):
    k, L, table = pr.make_vocabulary(3, 3, 3)
    pr.write_text(tmp_path / "v.txt", k, L, table)
    k1, L1, s1, w1, t1 = pr.read_text(tmp_path / "v.txt")
    assert (k1, L1, s1, w1) == (k, L, 0, 0) and t1.tobytes() == table.tobytes()  # repr() round-trips a double
    pr.write_binary(tmp_path / "v.bin", k1, L1, t1)
    k2, L2, s2, w2, t2 = pr.read_binary(tmp_path / "v.bin")
    assert (k2, L2, s2, w2) == (k, L, 0, 0)
    assert t2.tobytes() == pr.float_weights(table).tobytes()  # the binary form stores float weights
    assert not np.array_equal(t2["weight"], table["weight"])
    assert (tmp_path / "v.bin").stat().st_size == 24 + 41 * len(table)


def test_generators_plant_what_they_promise():
    k, L, table = pr.make_vocabulary(21, 10, 3)
    ids = np.arange(1, len(table) + 1)
    assert ((table["parent"] >= 0) & (table["parent"] < ids)).all()
    kids = np.bincount(table["parent"], minlength=len(table) + 1)
    assert kids.max() == k and ((kids[1:] == 0) == (table["is_leaf"] != 0)).all()
    assert (kids[np.r_[True, table["is_leaf"] == 0]] < k).any()  # inner nodes with fewer than k children
    depth = np.zeros(len(table) + 1, np.int64)
    for i in range(len(table)):
        depth[i + 1] = depth[table["parent"][i]] + 1
    leaf_depth = depth[1:][table["is_leaf"] != 0]
    assert leaf_depth.max() == L and (leaf_depth == 1).any() and (leaf_depth < L).any()
    assert (table["weight"][table["is_leaf"] != 0] == 0).any()
    assert (np.diff(table["parent"]) < 0).any()  # depth-first rows: children are not adjacent
    twins = sum(1 for i in range(1, len(table)) for j in range(i - 1, -1, -1)
                if table["parent"][j] == table["parent"][i] and (table["descriptor"][j] == table["descriptor"][i]).all())
    assert twins > 0
    keys = pr.make_descriptors(4, table, 300)
    assert len(np.unique(keys, axis=0)) < 300
    ref = br.RefVocabulary(k, L, table)
    w = [ref.transform_one(d, 1) for d in keys]
    assert any(wt == 0 for _, wt, _ in w) and len({x[0] for x in w}) < len(w)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
VOCS = [(10, 3, 1), (10, 3, 2), (3, 4, 2), (20, 2, 1), (10, 3, 4)]
_voc_cache = {}


def _voc(k, L):
    if (k, L) not in _voc_cache:
        _, _, table = pr.make_vocabulary(100 * k + L, k, L)
        _voc_cache[(k, L)] = (table, br.RefVocabulary(k, L, table))
    return _voc_cache[(k, L)]


def _assert_same(got, want, n_keys):
    ids, vals, fv = want
    node_id, node_first, node_feat = br.feat_arrays(fv)
    assert got.word_id.dtype == np.uint32 and np.array_equal(got.word_id, ids)
    assert np.array_equal(got.node_id, node_id)
    assert np.array_equal(got.node_first, node_first)
    assert np.array_equal(got.node_feat, node_feat)
    if len(ids):
        rel = np.abs(got.word_value - vals) / vals
        print("n_keys %d: %d words, %d nodes, word_value rel. error max %.3g" % (n_keys, len(ids), len(node_id), rel.max()))
        # any summation order of <= 8192 positive doubles is within 8191 * 2^-53 = 9.1e-13 of exact: once for the
        # reference's order, once for the device's, one rounding for the division
        assert rel.max() <= 2e-12


@pytest.mark.gpu
@pytest.mark.parametrize("k,L,levelsup", VOCS)
def test_transform_parity(k, L, levelsup):
    table, ref = _voc(k, L)
    voc = pr.Vocabulary(k, L, table)
    assert (voc.k, voc.L, voc.n_nodes, voc.n_words) == (k, L, len(table), ref.n_words)
    sizes = [65, 0, 1300, 1, 63]
    frames = [pr.make_descriptors(1000 + n, table, n) for n in sizes]
    batch = pr.transform(voc, frames, levelsup)  # 5 frames of unequal size in one call
    for n, f, got in zip(sizes, frames, batch):
        _assert_same(got, ref.transform(f, levelsup), n)
    for n in (64, 8192):  # batches of 1
        f = pr.make_descriptors(1000 + n, table, n)
        _assert_same(pr.transform(voc, [f], levelsup)[0], ref.transform(f, levelsup), n)
    assert len(batch[2].word_id) < 1300 and len(batch[2].node_first) > 1  # repeated words, stopped words


@pytest.mark.gpu
def test_transform_of_a_frame_whose_words_are_all_stopped():
    table, _ = _voc(10, 3)
    stopped = table.copy()
    stopped["weight"] = 0.0
    voc = pr.Vocabulary(10, 3, stopped)
    keys = pr.make_descriptors(9, table, 200)
    live = pr.Vocabulary(10, 3, table)
    a, b = pr.transform(voc, [keys], 1)[0], pr.transform(live, [keys], 1)[0]
    assert a.word_id.size == 0 and a.word_value.size == 0 and a.node_id.size == 0 and a.node_feat.size == 0
    assert a.node_first.tolist() == [0] and b.word_id.size > 0


@pytest.mark.gpu
def test_loading_table_text_and_binary_give_identical_transforms(tmp_path):
    k, L, levelsup = 10, 3, 1
    table, _ = _voc(k, L)
    keys = pr.make_descriptors(77, table, 700)
    pr.write_text(tmp_path / "voc.txt", k, L, table)
    pr.write_binary(tmp_path / "voc.bin", k, L, table)
    with open(tmp_path / "voc.txt", "a") as f:
        f.write("\n")  # the trailing empty line that gives the reference's loader its junk node
    from_table = pr.transform(pr.Vocabulary(k, L, table), [keys], levelsup)[0]
    from_text = pr.transform(pr.Vocabulary.load(tmp_path / "voc.txt"), [keys], levelsup)[0]
    from_float = pr.transform(pr.Vocabulary(k, L, pr.float_weights(table)), [keys], levelsup)[0]
    binary = pr.Vocabulary.load(tmp_path / "voc.bin")
    from_binary = pr.transform(binary, [keys], levelsup)[0]
    assert (binary.k, binary.L, binary.n_nodes) == (k, L, len(table))
    for a, b in ((from_table, from_text), (from_float, from_binary)):
        for name in ("word_id", "word_value", "node_id", "node_first", "node_feat"):
            assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert np.array_equal(from_table.word_id, from_binary.word_id)
    assert not np.array_equal(from_table.word_value, from_binary.word_value)  # float-rounded weights


@pytest.mark.gpu
def test_malformed_vocabularies_are_refused(tmp_path):
    L_ = _lib.lib()
    k, L, table = pr.make_vocabulary(8, 3, 2)

    def create(k=k, L=L, scoring=0, weighting=0, t=table):
        h = ctypes.c_void_p(0x5A5A)
        rc = L_.vieo_vocabulary_create(ctypes.byref(h), k, L, scoring, weighting, t.ctypes.data, len(t))
        return rc, h.value

    def load(path):
        h = ctypes.c_void_p(0x5A5A)
        return L_.vieo_vocabulary_load(ctypes.byref(h), str(path).encode()), h.value

    bad = (_lib.VIEO_E_INVALID, 0x5A5A)
    assert create(k=21) == bad and create(L=0) == bad and create(L=11) == bad  # bad header
    assert create(scoring=1) == bad and create(weighting=1) == bad  # unsupported
    t = table.copy()
    t["parent"][3] = 4  # parent >= own id (node 4)
    assert create(t=t) == bad
    t = table.copy()
    t["parent"][3] = -1
    assert create(t=t) == bad
    t = table.copy()
    t["is_leaf"][np.flatnonzero(table["is_leaf"] != 0)[0]] = 0  # an inner node without children
    assert create(t=t) == bad
    t = table.copy()
    t["is_leaf"][0] = 1  # a leaf with children
    assert create(t=t) == bad
    assert create(k=k - 1) == bad  # more than k children
    assert L_.vieo_vocabulary_create(None, k, L, 0, 0, table.ctypes.data, len(table)) == _lib.VIEO_E_INVALID
    pr.write_binary(tmp_path / "size.bin", k, L, table, size_node=40)
    pr.write_binary(tmp_path / "score.bin", k, L, table, scoring=2)
    pr.write_binary(tmp_path / "header.bin", 25, L, table)
    pr.write_text(tmp_path / "header.txt", k, 0, table)
    pr.write_text(tmp_path / "score.txt", k, L, table, weighting=1)
    pr.write_binary(tmp_path / "short.bin", k, L, table)
    with open(tmp_path / "short.bin", "r+b") as f:
        f.truncate(24 + 41 * len(table) - 7)
    t = table.copy()
    t["parent"][3] = 9
    pr.write_text(tmp_path / "parent.txt", k, L, t)
    for name in ("size.bin", "score.bin", "header.bin", "header.txt", "score.txt", "short.bin", "parent.txt", "missing.bin"):
        assert load(tmp_path / name) == bad, name
    pr.write_binary(tmp_path / "good.bin", k, L, table)
    rc, h = load(tmp_path / "good.bin")
    assert rc == _lib.VIEO_OK and h not in (None, 0x5A5A)
    L_.vieo_vocabulary_destroy(ctypes.c_void_p(h))


@pytest.mark.gpu
def test_transform_output_feeds_search_by_bow_as_it_is():
    """mFeatVec from vieo_bow_transform, passed as the node_* arrays of vieo_search_by_bow without repacking, gives the
    run where the same vectors come from the restatement"""
    from vieo_slam_amd import relocalization as rl
    k, L, levelsup = 10, 3, 2
    table, ref = _voc(k, L)
    voc = pr.Vocabulary(k, L, table)
    frame, kfs = rl.make_bow_scene(5, n_kfs=3, n_keys=300)
    everyone = [frame] + kfs
    got = pr.transform(voc, [b.desc for b in everyone], levelsup)
    direct = [rl.BowKeys.from_transform(b.keys, b.desc, g, b.mp_id) for b, g in zip(everyone, got)]
    restated = [rl.BowKeys(b.keys, b.desc, ref.transform(b.desc, levelsup)[2], b.mp_id) for b in everyone]
    a = rl.SearchByBoW(direct[1:], direct[0], 0.75, True)
    b = rl.SearchByBoW(restated[1:], restated[0], 0.75, True)
    assert len(a) == 3
    for (ma, na), (mb, nb) in zip(a, b):
        assert na == nb and np.array_equal(ma, mb)
    assert sum(n for _, n in a) > 30  # the scene's planted views are found through the vocabulary's nodes


@pytest.mark.gpu
def test_relocalization_from_place_recognition():
    """transform -> detect_reloc -> Relocalization: the helper's result is that of the existing call on the same
    candidates with mFeatVec from the restatement.  levelsup = L puts every key into node 0, so SearchByBoW sees all
    pairs of the scene (whose descriptors are random, not drawn from the vocabulary)."""
    from vieo_slam_amd import relocalization as rl
    k, L = 10, 3
    table, ref = _voc(k, L)
    voc = pr.Vocabulary(k, L, table)
    frame, cands, _ = rl.make_reloc_scene(3, "widen")
    descs = [frame.desc] + [c.bow.desc for c in cands]
    bows = pr.transform(voc, descs, L)
    restated = [ref.transform(d, L) for d in descs]
    db, want_db = pr.KeyFrameDatabase(voc), br.BatchedDatabase()
    for i, c in enumerate(cands):
        db.add(40 + i, bows[1 + i].word_id, bows[1 + i].word_value)
        want_db.add(40 + i, restated[1 + i][0], restated[1 + i][1])
    ids = db.detect_reloc(bows[0].word_id, bows[0].word_value)
    assert ids == want_db.detect_reloc(restated[0][0], restated[0][1]) and 40 in ids
    assert all(m > 1e-6 for m in want_db.margins)
    key_frames = {40 + i: rl.RelocCandidate(rl.BowKeys.from_transform(c.bow.keys, c.bow.desc, bows[1 + i], c.bow.mp_id), c.points)
                  for i, c in enumerate(cands)}
    got = rl.RelocalizationFromPlaceRecognition(bows[0], ids, key_frames, frame.keys, frame.uright, frame.desc, frame.K,
                                                frame.bf, frame.scale)
    frame2 = rl.RelocFrame(frame.keys, frame.uright, frame.desc, restated[0][2], frame.K, frame.bf, frame.scale)
    cands2 = [rl.RelocCandidate(rl.BowKeys(cands[i - 40].bow.keys, cands[i - 40].bow.desc, restated[1 + i - 40][2],
                                           cands[i - 40].bow.mp_id), cands[i - 40].points) for i in ids]
    want = rl.Relocalization(frame2, cands2)
    assert got["found"] and want["found"] and ids[got["cand"]] == 40
    assert got["cand"] == want["cand"] and got["n_good"] == want["n_good"]
    assert got["trace"].tobytes() == want["trace"].tobytes() and np.array_equal(got["Tcw"], want["Tcw"])
    assert np.array_equal(got["mp_ref"], want["mp_ref"]) and np.array_equal(got["outlier"], want["outlier"])
    none = rl.RelocalizationFromPlaceRecognition(bows[0], [], key_frames, frame.keys, frame.uright, frame.desc, frame.K,
                                                 frame.bf, frame.scale)
    assert not none["found"] and (none["mp_ref"] == -1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", DB_SIZES)
def test_database_parity(n):
    ref, margins = _reference_run(n)
    assert all(m > 1e-6 for m in margins)  # (asserted on the CPU before anything is compared)
    _, _, table = pr.make_vocabulary(77, 20, 3, early_leaf_share=0.0, short_share=0.0)
    voc = pr.Vocabulary(20, 3, table)
    assert voc.n_words >= DB_WORDS
    got = run_scenario(_Library(voc), _scene(n))
    assert len(got) == len(ref)
    for (what, a, tap_a), (_, b, tap_b) in zip(got, ref):
        if what.startswith("scores"):
            # sum |terms| <= 4, inputs within 2e-12 relative, plus the summation bound: 2e-11 absolute
            assert len(a) == len(b) and (len(b) == 0 or np.abs(a - b).max() <= 2e-11), what
            continue
        ids, n_common, first_word, score = tap_a
        assert ids.tolist() == tap_b[0] and n_common.tolist() == tap_b[1] and first_word.tolist() == tap_b[2], what
        if len(ids):
            err = np.abs(score - np.array(tap_b[3])).max()
            print("%s: %d key frames, score error max %.3g, list %s" % (what, len(ids), err, a[:6]))
            assert err <= 2e-11, what
        assert a == b, what


@pytest.mark.gpu
def test_invalid_arguments_write_nothing():
    L_ = _lib.lib()
    table, _ = _voc(10, 3)
    voc = pr.Vocabulary(10, 3, table)
    # transform: a frame above the cap, a null pointer
    rc, raw, out = pr.transform_call(voc, [pr.make_descriptors(1, table, 10), np.zeros((pr.MAX_KEYS + 1, 32), np.uint8)], 1)
    assert rc == _lib.VIEO_E_CAPACITY
    assert (out["n_words"] == -7).all() and (out["n_nodes"] == -7).all()
    for r in raw:
        assert (r.word_id == 0xDEADBEEF).all() and (r.word_value == -7.0).all() and (r.node_first == -7).all()
    assert L_.vieo_bow_transform(voc._h, None, 1, 1, out.ctypes.data) == _lib.VIEO_E_INVALID
    assert L_.vieo_bow_transform(None, None, 1, 1, out.ctypes.data) == _lib.VIEO_E_INVALID
    assert L_.vieo_bow_transform(voc._h, out.ctypes.data, 0, 1, out.ctypes.data) == _lib.VIEO_E_INVALID
    # database
    db = pr.KeyFrameDatabase(voc)
    rng = np.random.default_rng(2)
    q = br.random_bow(rng, voc.n_words, 60)
    for i in range(6):
        db.add(10 + i, *br.random_bow(rng, voc.n_words, 50, q, 0.8))
    assert db.add_call(12, *q) == _lib.VIEO_E_INVALID and len(db) == 6  # duplicate add
    assert db.erase_call(99) == _lib.VIEO_E_INVALID and len(db) == 6  # erase of an unknown id
    assert db.add_call(50, q[0][::-1].copy(), q[1]) == _lib.VIEO_E_INVALID  # words not ascending
    assert db.add_call(50, np.array([voc.n_words], np.uint32), np.ones(1)) == _lib.VIEO_E_INVALID and len(db) == 6
    want = db.detect_reloc(*q)
    assert len(want) >= 2
    tap = db.tap_query()
    rc, out_ids, n_out = db.detect_reloc_call(*q, 1)  # capacity too small
    assert rc == _lib.VIEO_E_CAPACITY and n_out == len(want) and (out_ids == -7).all()
    rc, out_ids, n_out = db.detect_loop_call(*q, [], 0.0, 0)
    assert rc == _lib.VIEO_E_CAPACITY and n_out >= 1 and (out_ids == -7).all()
    assert all(np.array_equal(x, y) for x, y in zip(tap, db.tap_query()))
    assert db.detect_reloc(*q) == want
    n = ctypes.c_int32(-7)
    w, v = q
    assert L_.vieo_kfdb_detect_reloc(db._h, None, v.ctypes.data, len(w), out_ids.ctypes.data, 6, ctypes.byref(n)) == _lib.VIEO_E_INVALID
    assert L_.vieo_kfdb_detect_reloc(db._h, w.ctypes.data, v.ctypes.data, len(w), out_ids.ctypes.data, 6, None) == _lib.VIEO_E_INVALID
    assert L_.vieo_kfdb_detect_reloc(None, w.ctypes.data, v.ctypes.data, len(w), out_ids.ctypes.data, 6, ctypes.byref(n)) == _lib.VIEO_E_INVALID
    assert n.value == -7 and (out_ids == -7).all()
    sc = np.full(2, -7.0)
    ids = np.array([10, 99], np.int64)
    assert L_.vieo_kfdb_scores(db._h, w.ctypes.data, v.ctypes.data, len(w), ids.ctypes.data, 2, sc.ctypes.data) == _lib.VIEO_E_INVALID
    assert (sc == -7.0).all()
    h = ctypes.c_void_p(0x5A5A)
    assert L_.vieo_kfdb_create(ctypes.byref(h), None) == _lib.VIEO_E_INVALID and h.value == 0x5A5A
    db.clear()
    assert len(db) == 0 and db.detect_reloc(*q) == []
