"""Place recognition on the device: the DBoW2 vocabulary (Vocabulary), FrameBase::ComputeBoW for a batch of frames
(transform) and KeyFrameDatabase with device-side scoring (KeyFrameDatabase); the writers of the reference's two
vocabulary file formats, and make_vocabulary / make_descriptors, the generators of the tests and of
tools/time_place_recognition.py."""
import ctypes
import struct

import numpy as np

from . import _lib

L1_NORM, TF_IDF = 0, 0
MAX_KEYS = 8192

VOC_NODE_DTYPE = np.dtype([("parent", np.int32), ("is_leaf", np.int32), ("descriptor", np.uint8, 32),
                           ("weight", np.float64)], align=True)
VOC_INFO_DTYPE = np.dtype([("k", np.int32), ("L", np.int32), ("n_nodes", np.int32), ("n_words", np.int32)], align=True)
BOW_FRAME_DTYPE = np.dtype([("n_keys", np.int32), ("reserved", np.int32), ("descriptors", np.uint64)], align=True)
BOW_VECTORS_DTYPE = np.dtype([("n_words", np.int32), ("n_nodes", np.int32), ("word_id", np.uint64),
                              ("word_value", np.uint64), ("node_id", np.uint64), ("node_first", np.uint64),
                              ("node_feat", np.uint64)], align=True)


# ---------------------------------------------------------------------------------------------------------------------
# the reference's files (TemplatedVocabulary::saveToTextFile / saveToBinaryFile)
def write_text(path, k, L, table, scoring=L1_NORM, weighting=TF_IDF):
    with open(path, "w") as f:
        f.write("%d %d  %d %d\n" % (k, L, scoring, weighting))
        for r in table:
            f.write("%d %d %s %r\n" % (r["parent"], 1 if r["is_leaf"] else 0, " ".join(str(int(b)) for b in r["descriptor"]),
                                       float(r["weight"])))


def write_binary(path, k, L, table, scoring=L1_NORM, weighting=TF_IDF, size_node=41):
    """weights are stored as float, as the reference's writer does"""
    with open(path, "wb") as f:
        f.write(struct.pack("<IIiiii", len(table) + 1, size_node, k, L, scoring, weighting))
        for r in table:
            f.write(struct.pack("<i", int(r["parent"])) + bytes(r["descriptor"]) +
                    struct.pack("<fB", float(r["weight"]), 1 if r["is_leaf"] else 0))


def read_text(path):
    """(k, L, scoring, weighting, table) of a text file; empty lines are skipped"""
    with open(path) as f:
        k, L, s, w = (int(v) for v in f.readline().split())
        rows = [ln.split() for ln in f if ln.strip()]
    table = np.zeros(len(rows), VOC_NODE_DTYPE)
    for i, r in enumerate(rows):
        table[i] = (int(r[0]), int(r[1]) > 0, [int(v) for v in r[2:34]], float(r[34]))
    return k, L, s, w, table


def read_binary(path):
    with open(path, "rb") as f:
        data = f.read()
    nb, size_node, k, L, s, w = struct.unpack_from("<IIiiii", data, 0)
    assert size_node == 41
    table = np.zeros(nb - 1, VOC_NODE_DTYPE)
    for i in range(nb - 1):
        o = 24 + 41 * i
        table[i] = (struct.unpack_from("<i", data, o)[0], data[o + 40] != 0, list(data[o + 4:o + 36]),
                    struct.unpack_from("<f", data, o + 36)[0])
    return k, L, s, w, table


def float_weights(table):
    """the table as it comes back from a binary file"""
    t = table.copy()
    t["weight"] = t["weight"].astype(np.float32).astype(np.float64)
    return t


# ---------------------------------------------------------------------------------------------------------------------
class Vocabulary:
    """vieo_vocabulary: the tree on the device.  Vocabulary(k, L, table) builds from a VOC_NODE_DTYPE table (node id =
    row + 1), Vocabulary.load(path) from one of the reference's files (".txt" in the name: text, else binary)."""

    def __init__(self, k=None, L=None, table=None, scoring=L1_NORM, weighting=TF_IDF, _handle=None):
        self._h = _handle
        if _handle is None:
            table = np.ascontiguousarray(table, VOC_NODE_DTYPE)
            h = ctypes.c_void_p()
            rc = _lib.lib().vieo_vocabulary_create(ctypes.byref(h), int(k), int(L), int(scoring), int(weighting),
                                                   table.ctypes.data if len(table) else None, len(table))
            _lib.check(rc, "vieo_vocabulary_create")
            self._h = h
        info = np.zeros(1, VOC_INFO_DTYPE)
        _lib.check(_lib.lib().vieo_vocabulary_info(self._h, info.ctypes.data), "vieo_vocabulary_info")
        self.k, self.L, self.n_nodes, self.n_words = (int(info[n][0]) for n in VOC_INFO_DTYPE.names)

    @classmethod
    def load(cls, path):
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().vieo_vocabulary_load(ctypes.byref(h), str(path).encode()), "vieo_vocabulary_load")
        return cls(_handle=h)

    def close(self):
        if self._h:
            _lib.lib().vieo_vocabulary_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BowResult:
    """One frame's mBowVec (word_id ascending, word_value) and mFeatVec (node_id ascending, node_first, node_feat -- the
    arrays vieo_bow_keys / vieo_tri_keyframe / vieo_reloc_frame take as they are)."""

    def __init__(self, word_id, word_value, node_id, node_first, node_feat):
        self.word_id, self.word_value = word_id, word_value
        self.node_id, self.node_first, self.node_feat = node_id, node_first, node_feat

    def feat_vec(self):
        """[(node id, [feature indices])], the form relocalization.BowKeys takes"""
        return [(int(n), [int(i) for i in self.node_feat[self.node_first[j]:self.node_first[j + 1]]])
                for j, n in enumerate(self.node_id)]


def transform_call(voc, frames, levelsup=4):
    """vieo_bow_transform, raw: (rc, [BowResult over the full-size output arrays], records)"""
    descs = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in frames]
    fr = np.zeros(len(descs), BOW_FRAME_DTYPE)
    out = np.zeros(len(descs), BOW_VECTORS_DTYPE)
    arrays = []
    for i, d in enumerate(descs):
        n = len(d)
        fr[i]["n_keys"] = n
        fr[i]["descriptors"] = d.ctypes.data if n else 0
        a = (np.full(max(n, 1), 0xDEADBEEF, np.uint32), np.full(max(n, 1), -7.0), np.full(max(n, 1), 0xDEADBEEF, np.uint32),
             np.full(n + 1, -7, np.int32), np.full(max(n, 1), -7, np.int32))
        arrays.append(a)
        out[i]["n_words"] = out[i]["n_nodes"] = -7
        for name, arr in zip(BOW_VECTORS_DTYPE.names[2:], a):
            out[i][name] = arr.ctypes.data
    rc = _lib.lib().vieo_bow_transform(voc._h, fr.ctypes.data if len(descs) else None, len(descs), int(levelsup),
                                       out.ctypes.data if len(descs) else None)
    return rc, [BowResult(*a) for a in arrays], out


def transform(voc, frames, levelsup=4):
    """FrameBase::ComputeBoW of every frame of the list (each (n, 32) uint8 descriptors) in one call.
    returns [BowResult]."""
    rc, raw, out = transform_call(voc, frames, levelsup)
    _lib.check(rc, "vieo_bow_transform")
    res = []
    for r, o in zip(raw, out):
        nw, nn = int(o["n_words"]), int(o["n_nodes"])
        res.append(BowResult(r.word_id[:nw].copy(), r.word_value[:nw].copy(), r.node_id[:nn].copy(),
                             r.node_first[:nn + 1].copy(), r.node_feat[:int(r.node_first[nn])].copy()))
    return res


class KeyFrameDatabase:
    """vieo_kfdb: the key frames' BowVectors on the device; DetectRelocalizationCandidates / DetectLoopCandidates."""

    def __init__(self, voc):
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().vieo_kfdb_create(ctypes.byref(h), voc._h), "vieo_kfdb_create")
        self._h, self._voc = h, voc

    def close(self):
        if self._h:
            _lib.lib().vieo_kfdb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return int(_lib.lib().vieo_kfdb_size(self._h))

    @staticmethod
    def _vec(word_id, word_value):
        w = np.ascontiguousarray(word_id, np.uint32)
        v = np.ascontiguousarray(word_value, np.float64)
        assert len(w) == len(v)
        return w, v

    def add_call(self, kf_id, word_id, word_value):
        w, v = self._vec(word_id, word_value)
        return _lib.lib().vieo_kfdb_add(self._h, int(kf_id), w.ctypes.data, v.ctypes.data, len(w))

    def add(self, kf_id, word_id, word_value):
        _lib.check(self.add_call(kf_id, word_id, word_value), "vieo_kfdb_add")

    def erase_call(self, kf_id):
        return _lib.lib().vieo_kfdb_erase(self._h, int(kf_id))

    def erase(self, kf_id):
        _lib.check(self.erase_call(kf_id), "vieo_kfdb_erase")

    def clear(self):
        _lib.check(_lib.lib().vieo_kfdb_clear(self._h), "vieo_kfdb_clear")

    def set_covisible(self, kf_id, ids):
        ids = np.ascontiguousarray(ids, np.int64)
        _lib.check(_lib.lib().vieo_kfdb_set_covisible(self._h, int(kf_id), ids.ctypes.data, len(ids)),
                   "vieo_kfdb_set_covisible")

    def scores(self, word_id, word_value, kf_ids):
        w, v = self._vec(word_id, word_value)
        ids = np.ascontiguousarray(kf_ids, np.int64)
        out = np.zeros(max(len(ids), 1))
        _lib.check(_lib.lib().vieo_kfdb_scores(self._h, w.ctypes.data, v.ctypes.data, len(w), ids.ctypes.data, len(ids),
                                               out.ctypes.data), "vieo_kfdb_scores")
        return out[:len(ids)]

    def detect_reloc_call(self, word_id, word_value, capacity):
        w, v = self._vec(word_id, word_value)
        out = np.full(max(capacity, 1), -7, np.int64)
        n = ctypes.c_int32(-7)
        rc = _lib.lib().vieo_kfdb_detect_reloc(self._h, w.ctypes.data, v.ctypes.data, len(w), out.ctypes.data, int(capacity),
                                               ctypes.byref(n))
        return rc, out, n.value

    def detect_reloc(self, word_id, word_value):
        """DetectRelocalizationCandidates: the key-frame ids, in the reference's order"""
        rc, out, n = self.detect_reloc_call(word_id, word_value, len(self))
        _lib.check(rc, "vieo_kfdb_detect_reloc")
        return [int(i) for i in out[:n]]

    def detect_loop_call(self, word_id, word_value, connected_ids, min_score, capacity):
        w, v = self._vec(word_id, word_value)
        conn = np.ascontiguousarray(connected_ids, np.int64)
        out = np.full(max(capacity, 1), -7, np.int64)
        n = ctypes.c_int32(-7)
        rc = _lib.lib().vieo_kfdb_detect_loop(self._h, w.ctypes.data, v.ctypes.data, len(w), conn.ctypes.data, len(conn),
                                              float(min_score), out.ctypes.data, int(capacity), ctypes.byref(n))
        return rc, out, n.value

    def detect_loop(self, word_id, word_value, connected_ids, min_score):
        """DetectLoopCandidates(pKF, minScore) with pKF->GetConnectedKeyFrames() = connected_ids"""
        rc, out, n = self.detect_loop_call(word_id, word_value, connected_ids, min_score, len(self))
        _lib.check(rc, "vieo_kfdb_detect_loop")
        return [int(i) for i in out[:n]]

    def tap_query(self):
        """test tap: (kf_ids, n_common, first_word, score) of the last query, key frames in insertion order"""
        n = len(self)
        ids, nc = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int32)
        fw, sc = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1))
        _lib.check(_lib.lib().vieo_kfdb_tap_query(self._h, ids.ctypes.data, nc.ctypes.data, fw.ctypes.data, sc.ctypes.data),
                   "vieo_kfdb_tap_query")
        return ids[:n], nc[:n], fw[:n], sc[:n]


# ---------------------------------------------------------------------------------------------------------------------
# generators
def _flip(rng, desc, nbits):
    d = desc.copy()
    for b in rng.choice(256, nbits, replace=False):
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


def make_vocabulary(seed, k=10, L=3, twin_share=0.1, short_share=0.15, early_leaf_share=0.08, stop_share=0.1,
                    order="depth"):
    """A seeded hierarchical vocabulary as a VOC_NODE_DTYPE table.  A child is its parent's descriptor with each bit
    flipped with probability (96 >> (depth - 1), at least 3) / 256, so fewer the deeper; twin_share of the children copy
    their elder sibling's descriptor exactly (ties the first must win); short_share of the inner nodes have fewer than k
    children; early_leaf_share of the nodes above depth L are leaves already (at any depth >= 1, so some lie above
    L - levelsup); stop_share of the words have weight 0.  order: "depth" = rows in depth-first order (a node's children
    are NOT adjacent rows), "breadth" = level by level.  returns (k, L, table)."""
    rng = np.random.default_rng(seed)
    parent_ids = np.zeros(1, np.int64)
    parent_desc = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    chunks, next_id = [], 1
    for depth in range(1, L + 1):
        m = len(parent_ids)
        n_kids = np.where(rng.random(m) >= short_share, k, rng.integers(1, k + 1, m))
        par = np.repeat(np.arange(m), n_kids)
        total = len(par)
        p = max(96 >> (depth - 1), 3) / 256.0
        desc = parent_desc[par] ^ np.packbits(rng.random((total, 256)) < p, axis=1)
        twin = np.flatnonzero((rng.random(total) < twin_share) & (np.arange(total) > 0) & (par == np.roll(par, 1)))
        for i in twin:  # ascending, so a twin of a twin copies the copy
            desc[i] = desc[i - 1]
        leaf = (rng.random(total) < early_leaf_share) | (depth == L)
        w = np.where(rng.random(total) < stop_share, 0.0, rng.uniform(0.5, 12.0, total))
        t = np.zeros(total, VOC_NODE_DTYPE)
        t["parent"], t["is_leaf"], t["descriptor"], t["weight"] = parent_ids[par], leaf, desc, np.where(leaf, w, 0.0)
        chunks.append(t)
        ids = next_id + np.arange(total)
        next_id += total
        parent_ids, parent_desc = ids[~leaf], desc[~leaf]
        if len(parent_ids) == 0:
            break
    table = np.concatenate(chunks)
    if order == "depth":
        n = len(table)
        first = np.zeros(n + 2, np.int64)
        np.add.at(first, table["parent"] + 1, 1)
        first = np.cumsum(first)  # rows are grouped by parent already: children of node p are rows first[p]..first[p + 1]
        new_id = np.zeros(n + 1, np.int64)
        seq, stack = [], [0]
        while stack:
            node = stack.pop()
            if node:
                new_id[node] = len(seq) + 1
                seq.append(node - 1)
            stack.extend(range(int(first[node + 1]), int(first[node]), -1))
        table = table[np.array(seq)]
        table["parent"] = new_id[table["parent"]]
    elif order != "breadth":
        raise ValueError("make_vocabulary: order is 'depth' or 'breadth'")
    return k, L, table


def make_descriptors(seed, table, n, noise_bits=6, duplicate_share=0.15):
    """n keys as noisy copies (0..noise_bits flipped bits) of the descriptors of random leaves of the table;
    duplicate_share of them repeat an earlier key exactly, so some words occur more than once.  returns (n, 32) uint8."""
    rng = np.random.default_rng(seed)
    leaves = np.flatnonzero(table["is_leaf"] != 0)
    out = np.zeros((n, 32), np.uint8)
    for i in range(n):
        if i > 0 and rng.uniform() < duplicate_share:
            out[i] = out[int(rng.integers(0, i))]
        else:
            out[i] = _flip(rng, table["descriptor"][leaves[int(rng.integers(0, len(leaves)))]], int(rng.integers(0, noise_bits + 1)))
    return out
