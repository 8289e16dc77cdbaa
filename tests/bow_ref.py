"""Restatement in Python of what vieo_bow_transform and vieo_kfdb compute (reference
loop/DBoW2/DBoW2/TemplatedVocabulary.h:1007-1129, BowVector.cpp:34-84, ScoringObject.cpp:23-68 and
src/KeyFrameDatabase.cc): RefVocabulary.transform, score, and the key-frame database twice -- LiteralDatabase walks an
inverted file with query stamps as the reference does, BatchedDatabase scores every key frame and orders the sharing
ones by (smallest shared word, insertion sequence) as the library does.  tests/test_place_recognition.py holds the two
against each other on the CPU and the library against BatchedDatabase on the GPU."""
import numpy as np

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
f32 = np.float32


class RefVocabulary:
    """table: VOC_NODE_DTYPE rows, node id = row + 1; children in row order; word ids in row order over the leaves"""

    def __init__(self, k, L, table):
        self.k, self.L = k, L
        n = len(table)
        self.children = [[] for _ in range(n + 1)]
        self.desc = np.zeros((n + 1, 32), np.uint8)
        self.weight = np.zeros(n + 1)
        self.word_id = np.full(n + 1, -1, np.int64)
        self.n_words = 0
        for i in range(n):
            nid = i + 1
            self.children[int(table["parent"][i])].append(nid)
            self.desc[nid], self.weight[nid] = table["descriptor"][i], table["weight"][i]
            if table["is_leaf"][i]:
                self.word_id[nid] = self.n_words
                self.n_words += 1
        self.kids = [np.array(c, np.int64) for c in self.children]

    def transform_one(self, d, levelsup):
        """transform(feature, word_id, weight, &nid, levelsup): (word id, weight, nid).  nid of a leaf above level
        L - levelsup, which the reference leaves uninitialised, is the leaf's own id."""
        nid_level = self.L - levelsup
        nid, final, level = 0, 0, 0
        while True:
            level += 1
            kids = self.kids[final]
            dist = _POP[self.desc[kids] ^ d].sum(axis=1)
            final = int(kids[int(np.argmin(dist))])  # the first of equal minima: the reference's strict <
            if level == nid_level:
                nid = final
            if len(self.kids[final]) == 0:
                break
        if level < nid_level:
            nid = final
        return int(self.word_id[final]), float(self.weight[final]), nid

    def transform(self, descs, levelsup):
        """(word_id uint32[], word_value float64[], [(node id, [feature indices ascending])])"""
        v, fv = {}, {}
        if self.n_words:
            for i, d in enumerate(np.asarray(descs, np.uint8).reshape(-1, 32)):
                w, wt, nid = self.transform_one(d, levelsup)
                if wt > 0:  # not stopped
                    v[w] = v.get(w, 0.0) + wt
                    fv.setdefault(nid, []).append(i)
        ids = sorted(v)
        vals = [v[w] for w in ids]
        norm = 0.0
        for x in vals:  # BowVector::normalize(L1), in the map's order
            norm += abs(x)
        if norm > 0.0:
            vals = [x / norm for x in vals]
        return np.array(ids, np.uint32), np.array(vals, np.float64), [(n, fv[n]) for n in sorted(fv)]


def score(ids1, vals1, ids2, vals2):
    """L1Scoring::score, the merge walk of ScoringObject.cpp:23-68"""
    i, j, s = 0, 0, 0.0
    n1, n2 = len(ids1), len(ids2)
    while i < n1 and j < n2:
        if ids1[i] == ids2[j]:
            vi, wi = float(vals1[i]), float(vals2[j])
            s += abs(vi - wi) - abs(vi) - abs(wi)
            i, j = i + 1, j + 1
        elif ids1[i] < ids2[j]:
            i = int(np.searchsorted(ids1, ids2[j]))
        else:
            j = int(np.searchsorted(ids2, ids1[i]))
    return -s / 2.0


def feat_arrays(fv):
    """[(node, [indices])] -> node_id, node_first, node_feat as the C-ABI lays them out"""
    node_id = np.array([n for n, _ in fv], np.uint32)
    node_first = np.zeros(len(fv) + 1, np.int32)
    node_first[1:] = np.cumsum([len(f) for _, f in fv])
    return node_id, node_first, np.array([i for _, f in fv for i in f], np.int32)


# ---------------------------------------------------------------------------------------------------------------------
class _KF:
    def __init__(self, kf_id, ids, vals):
        self.id, self.ids, self.vals = kf_id, np.asarray(ids, np.uint32), np.asarray(vals, np.float64)
        self.covis = []
        self.mnRelocQuery = self.mnLoopQuery = 0
        self.mnRelocWords = self.mnLoopWords = 0
        self.mRelocScore = self.mLoopScore = f32(0)  # (uninitialised in the reference: defined as 0)


class LiteralDatabase:
    """KeyFrameDatabase as written: mvInvertedFile (a list per word, in insertion order), the query stamps, the members
    on the key frames.  Every query gets a fresh id."""

    def __init__(self):
        self.inverted, self.kfs, self.query = {}, {}, 0

    def add(self, kf_id, ids, vals):
        kf = _KF(kf_id, ids, vals)
        self.kfs[kf_id] = kf
        for w in kf.ids:
            self.inverted.setdefault(int(w), []).append(kf)

    def erase(self, kf_id):
        kf = self.kfs.pop(kf_id)
        for w in kf.ids:
            self.inverted[int(w)].remove(kf)

    def set_covisible(self, kf_id, ids):
        self.kfs[kf_id].covis = list(ids)

    def _neighbours(self, kf):  # pointers to key frames that were erased (or never added) carry no stamp of this query
        return [self.kfs[i] for i in kf.covis if i in self.kfs]

    def detect_reloc(self, ids, vals):
        self.query += 1
        nid = self.query
        sharing = []
        for w in ids:
            for kf in self.inverted.get(int(w), []):
                if kf.mnRelocQuery != nid:
                    kf.mnRelocWords = 0
                    kf.mnRelocQuery = nid
                    sharing.append(kf)
                kf.mnRelocWords += 1
        if not sharing:
            return []
        maxCommonWords = max(kf.mnRelocWords for kf in sharing)
        minCommonWords = int(f32(maxCommonWords) * f32(0.8))
        lScoreAndMatch = []
        for kf in sharing:
            if kf.mnRelocWords > minCommonWords:
                si = f32(score(ids, vals, kf.ids, kf.vals))
                kf.mRelocScore = si
                lScoreAndMatch.append((si, kf))
        if not lScoreAndMatch:
            return []
        lAcc, bestAccScore = [], f32(0)
        for si, kf in lScoreAndMatch:
            bestScore, accScore, best = si, si, kf
            for kf2 in self._neighbours(kf):
                if kf2.mnRelocQuery != nid:
                    continue
                accScore = f32(accScore + kf2.mRelocScore)
                if kf2.mRelocScore > bestScore:
                    best, bestScore = kf2, kf2.mRelocScore
            lAcc.append((accScore, best))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = f32(f32(0.75) * bestAccScore)
        out = []
        for acc, kf in lAcc:
            if acc > minScoreToRetain and kf.id not in out:
                out.append(kf.id)
        return out

    def detect_loop(self, ids, vals, connected, min_score):
        self.query += 1
        nid, min_score, connected = self.query, f32(min_score), set(connected)
        sharing = []
        for w in ids:
            for kf in self.inverted.get(int(w), []):
                if kf.mnLoopQuery != nid:
                    kf.mnLoopWords = 0
                    if kf.id not in connected:
                        kf.mnLoopQuery = nid
                        sharing.append(kf)
                kf.mnLoopWords += 1
        if not sharing:
            return []
        maxCommonWords = max(kf.mnLoopWords for kf in sharing)
        minCommonWords = int(f32(maxCommonWords) * f32(0.8))
        lScoreAndMatch = []
        for kf in sharing:
            if kf.mnLoopWords > minCommonWords:
                si = f32(score(ids, vals, kf.ids, kf.vals))
                kf.mLoopScore = si
                if si >= min_score:
                    lScoreAndMatch.append((si, kf))
        if not lScoreAndMatch:
            return []
        lAcc, bestAccScore = [], min_score
        for si, kf in lScoreAndMatch:
            bestScore, accScore, best = si, si, kf
            for kf2 in self._neighbours(kf):
                if kf2.mnLoopQuery == nid and kf2.mnLoopWords > minCommonWords:
                    accScore = f32(accScore + kf2.mLoopScore)
                    if kf2.mLoopScore > bestScore:
                        best, bestScore = kf2, kf2.mLoopScore
            lAcc.append((accScore, best))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = f32(f32(0.75) * bestAccScore)
        out = []
        for acc, kf in lAcc:
            if acc > minScoreToRetain and kf.id not in out:
                out.append(kf.id)
        return out


class BatchedDatabase:
    """The library's formulation: per query, (shared words, smallest shared word, score) of EVERY stored key frame; the
    sharing ones ordered by (smallest shared word, insertion sequence); then the reference's tail.  `tap` holds the last
    query's table in insertion order, `margins` the distance of every threshold decision from its threshold."""

    def __init__(self):
        self.kfs, self.seq = [], 0  # insertion order
        self.tap, self.margins = None, []

    def add(self, kf_id, ids, vals):
        kf = _KF(kf_id, ids, vals)
        kf.seq = self.seq
        self.seq += 1
        self.kfs.append(kf)

    def erase(self, kf_id):
        self.kfs = [k for k in self.kfs if k.id != kf_id]

    def set_covisible(self, kf_id, ids):
        next(k for k in self.kfs if k.id == kf_id).covis = list(ids)

    def _table(self, ids, vals):
        ids = np.asarray(ids, np.uint32)
        tab = []
        for kf in self.kfs:
            shared = np.intersect1d(ids, kf.ids)
            tab.append((len(shared), int(shared[0]) if len(shared) else 0xFFFFFFFF, score(ids, vals, kf.ids, kf.vals)))
        self.tap = ([k.id for k in self.kfs], [t[0] for t in tab], [t[1] for t in tab], [t[2] for t in tab])
        return tab

    def scores(self, ids, vals, kf_ids):
        by_id = {k.id: k for k in self.kfs}
        return np.array([score(ids, vals, by_id[i].ids, by_id[i].vals) for i in kf_ids])

    def _detect(self, ids, vals, loop, connected, min_score):
        tab = self._table(ids, vals)
        connected, min_score = set(connected), f32(min_score)
        by_id = {k.id: j for j, k in enumerate(self.kfs)}
        listed = [j for j, k in enumerate(self.kfs) if tab[j][0] > 0 and not (loop and k.id in connected)]
        listed.sort(key=lambda j: (tab[j][1], self.kfs[j].seq))
        if not listed:
            return []
        is_listed = set(listed)
        maxCommonWords = max(tab[j][0] for j in listed)
        minCommonWords = int(f32(maxCommonWords) * f32(0.8))
        member = "mLoopScore" if loop else "mRelocScore"
        lScoreAndMatch = []
        for j in listed:
            if tab[j][0] > minCommonWords:
                si = f32(tab[j][2])
                setattr(self.kfs[j], member, si)
                if loop:
                    self.margins.append(abs(float(si) - float(min_score)))
                if not loop or si >= min_score:
                    lScoreAndMatch.append((si, j))
        if not lScoreAndMatch:
            return []
        lAcc, bestAccScore = [], min_score if loop else f32(0)
        for si, j in lScoreAndMatch:
            bestScore, accScore, best = si, si, j
            for i in self.kfs[j].covis:
                j2 = by_id.get(i)
                if j2 is None:
                    continue
                if loop and not (j2 in is_listed and tab[j2][0] > minCommonWords):
                    continue
                if not loop and tab[j2][0] == 0:
                    continue
                s2 = getattr(self.kfs[j2], member)
                accScore = f32(accScore + s2)
                self.margins.append(abs(float(s2) - float(bestScore)))
                if s2 > bestScore:
                    best, bestScore = j2, s2
            lAcc.append((accScore, best))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = f32(f32(0.75) * bestAccScore)
        out = []
        for acc, j in lAcc:
            self.margins.append(abs(float(acc) - float(minScoreToRetain)))
            if acc > minScoreToRetain and self.kfs[j].id not in out:
                out.append(self.kfs[j].id)
        return out

    def detect_reloc(self, ids, vals):
        return self._detect(ids, vals, False, (), 0.0)

    def detect_loop(self, ids, vals, connected, min_score):
        return self._detect(ids, vals, True, connected, min_score)


# ---------------------------------------------------------------------------------------------------------------------
def random_bow(rng, n_words_voc, n, base=None, keep=0.0):
    """an L1-normalised BowVector of n words below n_words_voc; a share `keep` of them (ids and roughly the values) from
    `base` = (ids, vals)"""
    ids, vals = [], []
    if base is not None and keep > 0:
        take = rng.choice(len(base[0]), min(int(keep * n), len(base[0])), replace=False)
        ids = [int(base[0][t]) for t in take]
        vals = [float(base[1][t]) * len(base[0]) * rng.uniform(0.5, 1.5) for t in take]
    free = np.setdiff1d(np.arange(n_words_voc), np.array(ids, np.int64))
    more = rng.choice(free, n - len(ids), replace=False)
    ids = np.concatenate([np.array(ids, np.int64), more])
    vals = np.concatenate([np.array(vals), rng.uniform(0.5, 12.0, len(more)) * rng.integers(1, 4, len(more))])
    order = np.argsort(ids)
    vals = vals[order] / vals.sum()
    return ids[order].astype(np.uint32), vals


def make_database_scene(seed, n_kfs, n_words_voc, lo=40, hi=400):
    """n_kfs key frames of lo..hi words from the lower 90 % of the vocabulary's words (so a query of the upper tenth shares
    nothing), two queries related to some of them, covisible lists of up to 10 ids that also name unknown ids, and a
    connected set.  returns dict(kfs = [(id, ids, vals)], covis = {id: [ids]}, queries = [(ids, vals)] * 2,
    nothing = (ids, vals), connected = [ids])."""
    rng = np.random.default_rng(seed)
    usable = int(n_words_voc * 0.9)
    hi = min(hi, usable // 2)
    queries = [random_bow(rng, usable, int(rng.integers(lo, hi + 1))) for _ in range(2)]
    kfs = []
    for i in range(n_kfs):
        base = queries[int(rng.integers(0, 2))] if rng.uniform() < 0.5 else None
        kfs.append((100 + 3 * i, *random_bow(rng, usable, int(rng.integers(lo, hi + 1)), base, rng.uniform(0.2, 0.9))))
    all_ids = [k[0] for k in kfs]
    covis = {}
    for kf_id in all_ids:
        if n_kfs > 1 and rng.uniform() < 0.8:
            c = [int(x) for x in rng.choice(all_ids, min(int(rng.integers(1, 11)), n_kfs - 1), replace=False) if x != kf_id]
            if rng.uniform() < 0.3:
                c.insert(int(rng.integers(0, len(c) + 1)), 7)  # an id that was never added
            covis[kf_id] = c[:10]
    top = np.arange(usable, n_words_voc)
    n_top = min(len(top), 30)
    nothing = (top[:n_top].astype(np.uint32), np.full(n_top, 1.0 / n_top))
    connected = [int(x) for x in rng.choice(all_ids, min(n_kfs // 4, 12), replace=False)] if n_kfs else []
    return dict(kfs=kfs, covis=covis, queries=queries, nothing=nothing, connected=connected)
