"""The symbolic part of the pose graph's tile-sparse LDL^T (vieo_slam_amd/csrc/pose_graph_plan.h) against a statement
made of sets: which key frames are unknowns, the blocks of H with their edges in edge order, tfirst[r] the leftmost tile
any block of tile row r touches, the row lists exactly the (r, k) with tfirst[r] <= k < r plus the right-hand side's
row, the envelope closed under fill, tile_off the prefix sum.  CPU only: the header is compiled with g++
(tests/emul/pose_graph_plan_emul.cc)."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TS = 64
_LISTS = ["col_of", "free_kf", "refs", "tfirst", "tile_off", "list_off", "rows"]


@functools.lru_cache(maxsize=None)
def plan_lib():
    out = os.path.join(HERE, "emul", "libpose_graph_plan_emul.so")
    deps = [os.path.join(HERE, "emul", "pose_graph_plan_emul.cc"), os.path.join(ROOT, "vieo_slam_amd", "csrc", "pose_graph_plan.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-o", out, deps[0]])
    return ctypes.CDLL(out)


def run_plan(valid, fixed_kf, ei, ej, pd):
    L = plan_lib()
    valid = np.ascontiguousarray(valid, np.uint8)
    ei, ej = np.ascontiguousarray(ei, np.int32), np.ascontiguousarray(ej, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    L.pgp_build(len(valid), p(valid), int(fixed_kf), len(ei), p(ei), p(ej), int(pd))
    h = np.zeros(6, np.int64)
    L.pgp_header(p(h))
    out = dict(zip(["pd", "n_free", "n", "T", "tiles", "n_items"], (int(v) for v in h)))
    for w, name in enumerate(_LISTS):
        a = np.zeros(L.pgp_len(w), np.int32)
        if len(a):
            L.pgp_get(w, p(a))
        out[name] = a
    items = np.zeros((out["n_items"], 5), np.int32)
    if len(items):
        L.pgp_items(p(items))
    out["items"] = items
    return out


def statement(valid, fixed_kf, ei, ej, pd):
    """the same plan from sets and dictionaries"""
    n_kf = len(valid)
    touched = set(ei) | set(ej)
    free = [k for k in range(n_kf) if valid[k] and k != fixed_kf and k in touched]
    col = {k: f for f, k in enumerate(free)}
    n = len(free) * pd
    T = (n + TS - 1) // TS
    # blocks (row vertex >= column vertex) -> [(edge, flag)] in edge order
    diag = {f: [] for f in range(len(free))}
    off = {}
    for e, (i, j) in enumerate(zip(ei, ej)):
        if i in col:
            diag[col[i]].append((e, 0))
        if j in col:
            diag[col[j]].append((e, 1))
        if i in col and j in col:
            # flag: the edge's vertex 0 is the block's column vertex
            off.setdefault((max(col[i], col[j]), min(col[i], col[j])), []).append((e, 1 if col[i] < col[j] else 0))
    blocks = [(f, f) for f in diag] + sorted(off)
    # the entries of the lower triangle's tiles that a block owns
    entries = {(rv * pd + a, cv * pd + b) for rv, cv in blocks for a in range(pd) for b in range(pd)}
    entries = {(r, c) for r, c in entries if r // TS >= c // TS}
    tfirst = [min([r] + [c // TS for rr, c in entries if rr // TS == r]) for r in range(T)]
    tiles = {(r, k) for r in range(T) for k in range(tfirst[r], r + 1)}
    lists = [[r for r in range(T) if tfirst[r] <= k < r] + [T] for k in range(T)]
    return dict(free=free, col=col, n=n, T=T, diag=diag, off=off, tfirst=tfirst, tiles=tiles, lists=lists, entries=entries)


def chain(n_kf):
    return [(k, k - 1) for k in range(1, n_kf)]


GRAPHS = {
    # name: (n_kf, edges (i, j), fixed_kf, invalid key frames)
    "chain": (30, chain(30), 0, ()),
    "chain-with-a-loop-edge": (40, chain(40) + [(39, 1)], 0, ()),
    "loop-edge-onto-the-fixed-vertex": (40, chain(40) + [(39, 0)], 0, ()),
    "comb-k-to-k-12": (70, chain(70) + [(k, k - 12) for k in range(12, 70)], 0, ()),
    "block-across-a-tile-boundary": (12, chain(12), 0, ()),
    "duplicate-edges": (25, chain(25) + [(7, 6), (6, 7), (20, 3), (20, 3), (3, 20)], 0, ()),
    "isolated-vertex": (25, [e for e in chain(25) if 11 not in e] + [(12, 10)], 0, ()),
    "invalid-vertex": (25, [e for e in chain(25) if 5 not in e] + [(6, 4)], 0, (5,)),
    "fixed-vertex-in-the-middle": (40, chain(40) + [(39, 2)], 17, ()),
    "two-components": (30, [e for e in chain(30) if e != (15, 14)], 0, ()),
    "single-free-vertex": (2, [(1, 0)], 0, ()),
    "exact-multiple-of-64": (33, chain(33) + [(32, 1)], 0, ()),
}


@pytest.mark.parametrize("pd", (6, 7))
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_plan_is_the_statement(name, pd):
    n_kf, edges, fixed, invalid = GRAPHS[name]
    valid = np.ones(n_kf, np.uint8)
    valid[list(invalid)] = 0
    ei, ej = [e[0] for e in edges], [e[1] for e in edges]
    P, S = run_plan(valid, fixed, ei, ej, pd), statement(valid, fixed, ei, ej, pd)
    T = S["T"]
    assert (P["pd"], P["n_free"], P["n"], P["T"]) == (pd, len(S["free"]), S["n"], T)
    assert list(P["free_kf"]) == S["free"] and [P["col_of"][k] for k in range(n_kf)] == [S["col"].get(k, -1) for k in range(n_kf)]
    # items: the diagonal blocks in vertex order, then the off-diagonal ones by (row, column) vertex; every block once
    want = [(1, f * pd, f * pd, S["diag"][f]) for f in sorted(S["diag"])] + [(0, rv * pd, cv * pd, S["off"][(rv, cv)]) for rv, cv in sorted(S["off"])]
    assert P["n_items"] == len(want)
    covered = np.zeros(len(P["refs"]), int)
    for it, (dg, rb, cb, refs) in zip(P["items"], want):
        assert tuple(it[:3]) == (dg, rb, cb)
        assert [(r >> 1, r & 1) for r in P["refs"][it[3]:it[4]]] == refs      # (duplicates: one block, its edges in edge order)
        covered[it[3]:it[4]] += 1
    assert (covered == 1).all()
    # the envelope
    assert list(P["tfirst"]) == S["tfirst"] + [0]
    counts = [r - S["tfirst"][r] + 1 for r in range(T)] + [T]
    assert list(P["tile_off"]) == [int(v) for v in np.concatenate([[0], np.cumsum(counts)])] and P["tiles"] == sum(counts)
    # every entry a block owns lies in a stored tile
    assert all((r // TS, c // TS) in S["tiles"] for r, c in S["entries"])
    # the lists: exactly the (r, k) with tfirst[r] <= k < r, ascending, then the right-hand side's row
    assert len(P["list_off"]) == T + 1 and P["list_off"][0] == 0
    for k in range(T):
        assert list(P["rows"][P["list_off"][k]:P["list_off"][k + 1]]) == S["lists"][k]
    assert len(P["rows"]) == P["list_off"][T]
    # closed under fill: whatever the update of column k writes exists
    for k in range(T):
        rows = S["lists"][k][:-1]
        for r in rows:
            for c in rows:
                if r >= c:
                    assert (r, c) in S["tiles"], (k, r, c)
    assert all((r, k) in S["tiles"] for k in range(T) for r in S["lists"][k][:-1])


def test_graphs_reach_what_they_are_for():
    pl = lambda name, pd: run_plan(np.ones(GRAPHS[name][0], np.uint8), GRAPHS[name][2], [e[0] for e in GRAPHS[name][1]],
                                   [e[1] for e in GRAPHS[name][1]], pd)
    P = pl("chain", 7)
    assert P["T"] == 4 and list(P["tfirst"][:4]) == [0, 0, 1, 2]                # a band: one tile back
    P = pl("chain-with-a-loop-edge", 7)
    assert P["T"] == 5 and P["tfirst"][4] == 0 and list(P["tfirst"][:4]) == [0, 0, 1, 2]     # the loop edge fills the last row only
    P = pl("loop-edge-onto-the-fixed-vertex", 7)
    assert P["tfirst"][4] == 3                                                     # an edge to the fixed vertex is no block
    P = pl("comb-k-to-k-12", 7)
    assert P["T"] == 8 and all(P["tfirst"][r] == max(0, r - 2) for r in range(8))   # 12 vertices back = 84 unknowns: two tiles
    for pd, f in ((7, 9), (6, 10)):
        P = pl("block-across-a-tile-boundary", pd)
        assert f * pd < TS < f * pd + pd - 1 and P["T"] == 2 and P["tfirst"][1] == 0
    P = pl("exact-multiple-of-64", 6)
    assert P["n"] == 192 and P["T"] == 3
    P = pl("single-free-vertex", 6)
    assert (P["n"], P["T"], P["tiles"]) == (6, 1, 2) and list(P["rows"]) == [1]
    P = pl("two-components", 6)
    assert P["n_free"] == 29 and P["n_items"] == 29 + 27
    P = pl("isolated-vertex", 7)
    assert P["col_of"][11] == -1 and P["n_free"] == 23
