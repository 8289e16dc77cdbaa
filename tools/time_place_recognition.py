"""Host-clock timing of the place-recognition entries on a generated k = 10, L = 6 vocabulary (about 1.1 million nodes):
vieo_bow_transform for 1 frame of 1200 keys and for 256 frames, vieo_kfdb_detect_reloc for 100 / 1000 / 5000 stored key
frames of about 1000 words, and, for scale, vieo_search_by_bow of 3 key frames of 1200 keys.  Each figure: WARMUP calls
unrecorded, then RUNS calls; median, minimum and 90th percentile in milliseconds.

    python tools/time_place_recognition.py [--runs 50] [--json out.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vieo_slam_amd import _lib  # noqa: E402
from vieo_slam_amd import place_recognition as pr  # noqa: E402
from vieo_slam_amd import relocalization as rl  # noqa: E402

WARMUP = 10


def clock(fn, runs):
    for _ in range(WARMUP):
        fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    t = np.sort(np.array(t))
    return dict(median_ms=float(np.median(t)), min_ms=float(t[0]), p90_ms=float(t[int(0.9 * (len(t) - 1))]), runs=runs)


def transform_closure(voc, frames, levelsup=4):
    """the bare C call on records built once (what a C++ caller pays)"""
    fr = np.zeros(len(frames), pr.BOW_FRAME_DTYPE)
    out = np.zeros(len(frames), pr.BOW_VECTORS_DTYPE)
    keep = []
    for i, d in enumerate(frames):
        n = len(d)
        fr[i]["n_keys"], fr[i]["descriptors"] = n, d.ctypes.data
        a = (np.zeros(n, np.uint32), np.zeros(n), np.zeros(n, np.uint32), np.zeros(n + 1, np.int32), np.zeros(n, np.int32))
        keep.append(a)
        for name, arr in zip(pr.BOW_VECTORS_DTYPE.names[2:], a):
            out[i][name] = arr.ctypes.data
    f = _lib.lib().vieo_bow_transform

    def call():
        _lib.check(f(voc._h, fr.ctypes.data, len(frames), levelsup, out.ctypes.data), "vieo_bow_transform")

    return call, out, keep, fr


def random_vectors(rng, n_words_voc, n_kfs, query, n=1000):
    vecs = []
    for i in range(n_kfs):
        ids = rng.integers(0, n_words_voc, n + n // 8)
        if i % 2 == 0:  # every other key frame has seen the query's place
            ids = np.concatenate([ids, rng.choice(query[0], len(query[0]) // 3, replace=False)])
        ids = np.unique(ids)[:n].astype(np.uint32)
        vals = rng.uniform(0.5, 12.0, len(ids))
        vecs.append((ids, vals / vals.sum()))
    return vecs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    res = {}
    t0 = time.perf_counter()
    k, L, table = pr.make_vocabulary(1, 10, 6, short_share=0.0, early_leaf_share=0.0, order="breadth")
    voc = pr.Vocabulary(k, L, table)
    res["vocabulary"] = dict(k=k, L=L, n_nodes=voc.n_nodes, n_words=voc.n_words, build_s=time.perf_counter() - t0,
                             library=os.path.basename(_lib.LIB_PATH))
    distinct = [pr.make_descriptors(10 + i, table, 1200) for i in range(16)]
    call, out, keep, _ = transform_closure(voc, distinct[:1])
    res["transform_1x1200"] = clock(call, args.runs)
    res["transform_1x1200"]["n_words"] = int(out[0]["n_words"])
    call, _, keep2, _ = transform_closure(voc, [distinct[i % 16] for i in range(256)])
    res["transform_256x1200"] = clock(call, max(args.runs // 5, 5))
    big = pr.make_descriptors(99, table, 6000)
    call, _, keep3, _ = transform_closure(voc, [big])
    res["transform_1x6000"] = clock(call, args.runs)
    # the database
    rng = np.random.default_rng(3)
    q = pr.transform(voc, distinct[:1])[0]
    query = (q.word_id, q.word_value)
    for n_kfs in (100, 1000, 5000):
        db = pr.KeyFrameDatabase(voc)
        for i, (ids, vals) in enumerate(random_vectors(rng, voc.n_words, n_kfs, query)):
            db.add(i, ids, vals)
        for i in range(0, n_kfs, 3):
            db.set_covisible(i, [(i + j) % n_kfs for j in range(1, 11)])
        w, v = db._vec(*query)
        ids_out, n_out = np.zeros(n_kfs, np.int64), ctypes.c_int32()
        f = _lib.lib().vieo_kfdb_detect_reloc

        def detect():
            _lib.check(f(db._h, w.ctypes.data, v.ctypes.data, len(w), ids_out.ctypes.data, n_kfs, ctypes.byref(n_out)),
                       "vieo_kfdb_detect_reloc")

        res["detect_reloc_%d" % n_kfs] = clock(detect, args.runs)
        res["detect_reloc_%d" % n_kfs].update(query_words=len(w), candidates=n_out.value)
        db.close()
    # for scale: SearchByBoW of 3 key frames of 1200 keys against a frame of 1200
    frame, kfs = rl.make_bow_scene(5, n_kfs=3, n_keys=1200, n_nodes=100)
    res["search_by_bow_3x1200"] = clock(lambda: rl.SearchByBoW(kfs, frame, 0.75, True), args.runs)
    for name, r in res.items():
        print(name, json.dumps(r))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
