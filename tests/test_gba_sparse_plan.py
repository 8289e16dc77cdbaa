"""Symbolic plan of the full BA's tile-sparse LDL^T (vieo_slam_amd/csrc/gba_sparse_plan.h) against a numpy restatement:
the element pattern of the reduced system and of the visual Schur product, cut into 64 x 64 tiles, closed under
boolean tile elimination.  CPU only: the header is compiled with g++ into a small library here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from vieo_slam_amd import synth_ba

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 64

_SHIM = r"""
#include "gba_sparse_plan.h"
static vieo::GbaSparsePlan g_plan;
extern "C" void plan_build(int n_kf, const int* fixed, int n_obs, const int* okf, const int* omp, int n_mp, int n_pair,
                           const int* pi, const int* pj, int pd, int sco) {
  vieo::gba_sparse_plan(g_plan, n_kf, fixed, n_obs, okf, omp, n_mp, n_pair, pi, pj, pd, sco);
}
extern "C" void plan_header(long long* h) {
  const vieo::GbaSparsePlan& P = g_plan;
  const long long v[12] = {P.nf, P.n, P.nt, P.vrb, P.vcb, (long long)P.n_sch_tiles(), (long long)P.n_tiles(),
                           (long long)(P.upd.size() / 5), (long long)P.bytes(1), (long long)P.pool_bytes(),
                           (long long)P.list_ints(), (long long)P.bytes(3)};
  for (int i = 0; i < 12; i++) h[i] = v[i];
}
static const std::vector<int>& pick(int w) {
  const vieo::GbaSparsePlan& P = g_plan;
  const std::vector<int>* l[] = {&P.col_of, &P.sch_ptr, &P.sch_i, &P.sch_j, &P.sch_diag, &P.sch_off, &P.col_ptr,
                                 &P.tile_i, &P.tile_j, &P.row_ptr, &P.row_j, &P.row_tile, &P.upd_ptr, &P.upd};
  return *l[w];
}
extern "C" int plan_len(int w) { return (int)pick(w).size(); }
extern "C" void plan_get(int w, int* out) { for (size_t i = 0; i < pick(w).size(); i++) out[i] = pick(w)[i]; }
"""
_NAMES = ["col_of", "sch_ptr", "sch_i", "sch_j", "sch_diag", "sch_off", "col_ptr", "tile_i", "tile_j", "row_ptr", "row_j",
          "row_tile", "upd_ptr", "upd"]


@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("gba_plan")
    src, so = d / "shim.cc", d / "libgbaplan.so"
    src.write_text(_SHIM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC",
                           "-I" + os.path.join(ROOT, "vieo_slam_amd", "csrc"), str(src), "-o", str(so)])
    return ctypes.CDLL(str(so))


def run_plan(lib, fixed, okf, omp, n_mp, pairs, pd, sco):
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    fixed, okf, omp = i32(fixed), i32(okf), i32(omp)
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    pi, pj = i32(pairs[:, 0]), i32(pairs[:, 1])
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    lib.plan_build(len(fixed), p(fixed), len(okf), p(okf), p(omp), n_mp, len(pairs), p(pi), p(pj), pd, sco)
    h = np.zeros(12, np.int64)
    lib.plan_header(h.ctypes.data_as(ctypes.c_void_p))
    out = dict(zip(["nf", "n", "nt", "vrb", "vcb", "n_sch", "n_tiles", "n_upd", "bytes1", "pool", "ints", "bytes3"],
                   (int(x) for x in h)))
    for w, name in enumerate(_NAMES):
        a = np.zeros(lib.plan_len(w), np.int32)
        if len(a):
            lib.plan_get(w, a.ctypes.data_as(ctypes.c_void_p))
        out[name] = a
    return out


def reference(fixed, okf, omp, n_mp, pairs, pd, sco):
    """(column of every key frame, upper Schur tile pattern [vrb, vcb], filled lower tile pattern [nt, nt])"""
    n_kf = len(fixed)
    k = np.asarray(okf) & 0xFFFFFF
    ok = (np.asarray(okf) >= 0) & (k < n_kf) & (np.asarray(omp) >= 0) & (np.asarray(omp) < n_mp)
    k, m = k[ok], np.asarray(omp)[ok]
    act = np.zeros(n_kf, bool)
    act[k] = True
    pairs = np.asarray(pairs, int).reshape(-1, 2)
    if pd == 6 and len(pairs):
        act[pairs.ravel()] = True
    col = -np.ones(n_kf, int)
    free = (np.asarray(fixed) == 0) & (act | (pd == 15))
    col[free] = np.arange(free.sum())
    nf = int(free.sum())
    npv, n = 6 * nf + sco, pd * nf + sco
    # visual: BB pattern (rows of the 6 nf + sco grid x points), its Gram pattern, the b_l column (dense in k_lba_schur)
    BB = np.zeros((npv, max(n_mp, 1)), bool)
    for kk, mm in zip(k, m):
        if col[kk] >= 0:
            BB[6 * col[kk]:6 * col[kk] + 6, mm] = True
    if sco:
        BB[npv - 1, np.unique(m)] = True
    S = (BB.astype(np.int64) @ BB.T.astype(np.int64)) > 0
    vrb, vcb = -(-npv // T), (npv + T) // T
    St = np.zeros((vrb, vcb), bool)
    for bi in range(vrb):
        for bj in range(bi, min(vcb, vrb)):
            St[bi, bj] = S[bi * T:(bi + 1) * T, bj * T:(bj + 1) * T].any()
    St[:, vcb - 1] = True
    # reduced system, bordered: (n + 1) x (n + 1) element pattern
    A = np.zeros((n + 1, n + 1), bool)
    for a in range(nf):
        A[pd * a:pd * a + pd, pd * a:pd * a + pd] = True
    cov = (BB[:6 * nf].reshape(nf, 6, -1).any(1).astype(np.int64) @ BB[:6 * nf].reshape(nf, 6, -1).any(1).T.astype(np.int64)) > 0
    for a, b in zip(*np.nonzero(cov)):
        A[pd * a:pd * a + 6, pd * b:pd * b + 6] = True
    for i, j in pairs:
        if col[i] >= 0 and col[j] >= 0:
            A[pd * col[i]:pd * col[i] + pd, pd * col[j]:pd * col[j] + pd] = True
            A[pd * col[j]:pd * col[j] + pd, pd * col[i]:pd * col[i] + pd] = True
    if sco:
        A[n - 1, :n] = A[:n, n - 1] = True
    A[n, :] = A[:, n] = True
    nt = -(-(n + 1) // T)
    R = np.zeros((nt, nt), bool)
    for I in range(nt):
        for J in range(I + 1):
            R[I, J] = A[I * T:(I + 1) * T, J * T:(J + 1) * T].any() or I == J
    for kk in range(nt):  # boolean tile elimination
        rows = kk + 1 + np.nonzero(R[kk + 1:, kk])[0]
        R[np.ix_(rows, rows)] = True
    return col, St, np.tril(R)


def check_plan(P, fixed, okf, omp, n_mp, pairs, pd, sco):
    col, St, R = reference(fixed, okf, omp, n_mp, pairs, pd, sco)
    nt = R.shape[0]
    assert np.array_equal(P["col_of"], col)
    assert P["nt"] == nt and P["n"] == pd * P["nf"] + sco and (P["vrb"], P["vcb"]) == St.shape
    # Schur tiles: row by row, bj ascending; the diagonal / off-diagonal index lists partition them
    got = np.zeros_like(St)
    got[P["sch_i"], P["sch_j"]] = True
    assert np.array_equal(got, St) and P["n_sch"] == St.sum()
    assert np.all(np.diff(P["sch_i"] * 100000 + P["sch_j"]) > 0)
    assert np.array_equal(np.bincount(P["sch_i"], minlength=St.shape[0]), np.diff(P["sch_ptr"]))
    assert np.array_equal(np.sort(np.r_[P["sch_diag"], P["sch_off"]]), np.arange(P["n_sch"]))
    assert np.all(P["sch_i"][P["sch_diag"]] == P["sch_j"][P["sch_diag"]])
    assert np.all(P["sch_i"][P["sch_off"]] < P["sch_j"][P["sch_off"]])
    # reduced tiles: the filled pattern, column by column with the diagonal first; slot = position
    got = np.zeros_like(R)
    got[P["tile_i"], P["tile_j"]] = True
    assert np.array_equal(got, R) and P["n_tiles"] == R.sum()
    slot = -np.ones((nt, nt), int)
    slot[P["tile_i"], P["tile_j"]] = np.arange(P["n_tiles"])
    for J in range(nt):
        c = np.arange(P["col_ptr"][J], P["col_ptr"][J + 1])
        assert np.all(P["tile_j"][c] == J) and P["tile_i"][c[0]] == J and np.all(np.diff(P["tile_i"][c]) > 0)
    assert P["tile_i"][P["col_ptr"][:-1]].tolist() == list(range(nt))
    assert R[nt - 1].all(), "the right-hand-side row is full"
    for I in range(nt):  # back-substitution rows: column ascending, diagonal last, slots of the same tiles
        r = np.arange(P["row_ptr"][I], P["row_ptr"][I + 1])
        assert np.array_equal(P["row_j"][r], np.nonzero(R[I, :I + 1])[0]) and P["row_j"][r[-1]] == I
        assert np.array_equal(P["row_tile"][r], slot[I, P["row_j"][r]])
    # update targets: every (i, j) pair below panel k, each existing, with the slots of (i, k), (j, k), (i, j)
    U = P["upd"].reshape(-1, 5)
    assert len(U) == P["n_upd"] and P["upd_ptr"][-1] == len(U)
    for kk in range(nt):
        rows = np.nonzero(R[kk + 1:, kk])[0] + kk + 1
        u = U[P["upd_ptr"][kk]:P["upd_ptr"][kk + 1]]
        want = {(i, j) for i in rows for j in rows if j <= i}
        assert {(int(a), int(b)) for a, b in u[:, :2]} == want and len(u) == len(want)
        assert np.all(u[:, 4] >= 0) and np.all(slot[u[:, 0], u[:, 1]] == u[:, 4])
        assert np.all(slot[u[:, 0], kk] == u[:, 2]) and np.all(slot[u[:, 1], kk] == u[:, 3])
    # byte count: pool + Schur partials per split + the panel's W + the lists
    tile_b = T * T * 8
    assert P["pool"] == P["n_tiles"] * tile_b
    assert P["bytes1"] == P["pool"] + P["n_sch"] * tile_b + nt * tile_b + 4 * P["ints"]
    assert P["bytes3"] - P["bytes1"] == 2 * P["n_sch"] * tile_b
    return R


def banded(rng, n_kf, n_mp, span, n_fixed=1, loop=0):
    """index-only observations: every point seen by a few key frames within `span` of its anchor (+ `loop` points seen
    by an early and a late one); the fixed key frames (last) see the first points"""
    n_loc = n_kf - n_fixed
    okf, omp = [], []
    for m in range(n_mp):
        a = rng.integers(0, n_loc)
        ks = np.unique(np.clip(a + rng.integers(-span, span + 1, rng.integers(2, 5)), 0, n_loc - 1))
        okf += ks.tolist()
        omp += [m] * len(ks)
    for t in range(n_fixed):
        okf += [n_loc + t] * 5
        omp += list(range(5))
    for t in range(loop):
        okf += [int(rng.integers(0, n_loc // 4)), int(rng.integers(3 * n_loc // 4, n_loc))]
        omp += [n_mp + t] * 2
    o = np.argsort(omp, kind="stable")
    fixed = np.r_[np.zeros(n_loc, int), np.ones(n_fixed, int)]
    return fixed, np.asarray(okf)[o], np.asarray(omp)[o], n_mp + loop


def chain(n_loc, n_fixed=1):
    return [(n_loc, 0)] + [(k - 1, k) for k in range(1, n_loc)] if n_fixed else [(k - 1, k) for k in range(1, n_loc)]


@pytest.mark.parametrize("pd,sco,n_kf,span,loop", [
    (15, 1, 120, 3, 0),   # banded VIO with the scale row (1801 unknowns)
    (15, 0, 90, 5, 0),    # banded VIO
    (15, 1, 150, 3, 4),   # loop closure: fill far off the band
    (6, 0, 400, 4, 0),    # vision only
    (6, 1, 300, 4, 3),    # vision only, scale row, loop
])
def test_plan_matches_numpy_reference(plan_lib, pd, sco, n_kf, span, loop):
    rng = np.random.default_rng(n_kf + 7 * loop)
    fixed, okf, omp, n_mp = banded(rng, n_kf, 3 * n_kf, span, loop=loop)
    pairs = chain(n_kf - 1) if pd == 15 else []
    P = run_plan(plan_lib, fixed, okf, omp, n_mp, pairs, pd, sco)
    R = check_plan(P, fixed, okf, omp, n_mp, pairs, pd, sco)
    nt = R.shape[0]
    assert R.sum() < nt * (nt + 1) // 2, "a banded trajectory stores a fraction of the triangle"
    if loop:  # the loop's fill: tiles far below the band of the same trajectory without it
        f0, k0, m0, n0 = banded(np.random.default_rng(n_kf + 7 * loop), n_kf, 3 * n_kf, span)
        assert R.sum() > run_plan(plan_lib, f0, k0, m0, n0, pairs, pd, sco)["n_tiles"]


def test_plan_free_key_frame_without_observations(plan_lib):
    """Vision only: a free key frame nobody observes from has no column (k_lba_begin); visual-inertial: it keeps one.
    Camera bits (kf >> 24) are masked off; out-of-range observations are ignored."""
    rng = np.random.default_rng(3)
    fixed, okf, omp, n_mp = banded(rng, 60, 150, 3)
    keep = okf != 17
    okf, omp = okf[keep].copy(), omp[keep]
    okf[::3] |= 1 << 24
    okf, omp = np.r_[okf, 70, 5], np.r_[omp, 10, n_mp + 3]  # key frame out of range, point out of range
    P = run_plan(plan_lib, fixed, okf, omp, n_mp, [], 6, 0)
    assert P["col_of"][17] == -1 and P["nf"] == 58 and P["col_of"][18] == 17
    check_plan(P, fixed, okf, omp, n_mp, [], 6, 0)
    P = run_plan(plan_lib, fixed, okf, omp, n_mp, chain(59), 15, 1)
    assert P["col_of"][17] == 17 and P["nf"] == 59
    check_plan(P, fixed, okf, omp, n_mp, chain(59), 15, 1)
    # encoder pairs make a vision-only key frame active
    P = run_plan(plan_lib, fixed, okf, omp, n_mp, [(16, 17), (17, 18)], 6, 0)
    assert P["col_of"][17] == 17
    check_plan(P, fixed, okf, omp, n_mp, [(16, 17), (17, 18)], 6, 0)


@pytest.mark.parametrize("nf", [10, 11, 21, 32, 42, 43, 64])
def test_plan_key_frame_straddling_tiles(plan_lib, nf):
    """6 nf: the last key frame's six rows straddle a 64-row tile (nf = 11: rows 60..65), and the right-hand-side row
    opens a tile of its own when pd nf + sco is a multiple of 64 (nf = 32, 64)."""
    rng = np.random.default_rng(nf)
    fixed, okf, omp, n_mp = banded(rng, nf + 1, 4 * nf, 2)
    for sco in (0, 1):
        P = run_plan(plan_lib, fixed, okf, omp, n_mp, [], 6, sco)
        check_plan(P, fixed, okf, omp, n_mp, [], 6, sco)


@pytest.mark.parametrize("seed", range(6))
def test_plan_random_patterns(plan_lib, seed):
    """Random covisibility (any key frame with any other), random fixed ones, random pair edges."""
    rng = np.random.default_rng(100 + seed)
    n_kf, n_mp = int(rng.integers(8, 90)), int(rng.integers(20, 200))
    fixed = (rng.random(n_kf) < 0.15).astype(int)
    okf, omp = [], []
    for m in range(n_mp):
        ks = np.unique(rng.integers(0, n_kf, rng.integers(1, 4)))
        okf += ks.tolist()
        omp += [m] * len(ks)
    pd, sco = [(6, 0), (6, 1), (15, 0), (15, 1)][seed % 4]
    perm = rng.permutation(n_kf)
    pairs = [(int(perm[t]), int(perm[t + 1])) for t in range(0, n_kf - 1, 2)]
    P = run_plan(plan_lib, fixed, okf, omp, n_mp, pairs, pd, sco)
    check_plan(P, fixed, okf, omp, n_mp, pairs, pd, sco)


def test_plan_of_a_synthetic_loop_problem(plan_lib):
    """synth_ba's loop option: the plan of a visual-inertial map with a loop closure has fill the banded one has not;
    the default problem is unchanged by the option's existence."""
    a = synth_ba.make_lba_vio_problem(21, n_local=60, n_fixed=1, n_points=3000, anchors=30, span=5)
    b = synth_ba.make_lba_vio_problem(21, n_local=60, n_fixed=1, n_points=3000, anchors=30, span=5, loop=40)
    n0 = len(a[2])
    assert len(b[2]) > n0 and np.array_equal(b[2][:n0], a[2]) and np.array_equal(b[4][:len(a[4])], a[4])
    assert np.all(b[4]["mp"][len(a[4]):] >= n0) and np.all(np.diff(b[4]["mp"]) >= 0)
    plans = []
    for (params, kfs, pts, close, obs, imu, gt) in (a, b):
        args = (kfs["fixed"], obs["kf"], obs["mp"], len(pts), np.c_[imu["kf_i"], imu["kf_j"]], 15, 1)
        P = run_plan(plan_lib, *args)
        check_plan(P, *args)
        plans.append(P)
    assert plans[1]["n_tiles"] > plans[0]["n_tiles"]
