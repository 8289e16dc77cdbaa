"""The host half of the PnP and Sim3 RANSAC handles (vieo_slam_amd/csrc/ransac_table.h): the sample filler and its draw,
the tail of SetRansacParameters, the candidate layout, the row tables, PnP's record selection and the two replays of
iterate, fed with synthetic tables (counts, masks, poses of random doubles) and compared call by call with the Python
restatements that the GPU tests use: reloc_ref.IterateReplay and loop_ref.Sim3SolverRef(tables=...).  CPU only: the
header is compiled with g++ (tests/emul/ransac_table_emul.cc); the device fills the same tables in
test_relocalization*.py and test_loop_sim3*.py."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import loop_ref, reloc_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
VIEO_OK, VIEO_E_CAPACITY, VIEO_E_EMPTY = 0, -4, -5
PNP, SIM3 = 0, 1
POSE = {PNP: 12, SIM3: 13}
PLANTED = (0, 63, 64, 128)  # inliers on both sides of the mask words' boundaries


class PnpParams(ctypes.Structure):
    _fields_ = [("probability", ctypes.c_double), ("min_inliers", ctypes.c_int32), ("max_iterations", ctypes.c_int32),
                ("min_set", ctypes.c_int32), ("epsilon", ctypes.c_float), ("th2", ctypes.c_float), ("reserved", ctypes.c_int32)]


class Sim3Params(ctypes.Structure):
    _fields_ = [("probability", ctypes.c_double), ("min_inliers", ctypes.c_int32), ("max_iterations", ctypes.c_int32)]


@functools.lru_cache(maxsize=None)
def lib():
    out = os.path.join(HERE, "emul", "libransac_table_emul.so")
    deps = [os.path.join(HERE, "emul", "ransac_table_emul.cc"), os.path.join(ROOT, "vieo_slam_amd", "csrc", "ransac_table.h"),
            os.path.join(ROOT, "include", "vieo_hot.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-o", out, deps[0]])
    L = ctypes.CDLL(out)
    L.rt_error.restype = ctypes.c_char_p
    L.rt_draw.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.rt_max_iterations.argtypes = [ctypes.c_double, ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    for f in (L.rt_pnp_new, L.rt_sim3_new):
        f.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    return L


def p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def pack(mask):
    """bool (rows, n) -> uint64 (rows, words), bit i of word i // 64 = correspondence i"""
    rows, n = mask.shape
    padded = np.zeros((rows, (n + 63) // 64 * 64), np.uint8)
    padded[:, :n] = mask
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint64).reshape(rows, -1)


def masks_with(rng, n, counts):
    """one mask row per count: the planted bits first, as many as the count allows, then random others"""
    out = np.zeros((len(counts), n), bool)
    for r, k in enumerate(counts):
        first = [b for b in PLANTED if b < n][:k]
        rest = rng.permutation(np.setdiff1d(np.arange(n), first))[:k - len(first)]
        out[r, first] = True
        out[r, rest] = True
    assert (out.sum(axis=1) == counts).all()
    return out


class Handle:
    """one emulated handle: K candidates of n[c] correspondences, their index maps into n_out[c] > n[c] entries"""

    def __init__(self, which, n, params, S, samples=None, seed=5, rng=None):
        rng = rng or np.random.default_rng(1)
        self.which, self.n, self.S, self.K = which, list(n), S, len(n)
        self.n_out = [k + 37 for k in self.n]
        self.index = [rng.permutation(o)[:k].astype(np.int32) for k, o in zip(self.n, self.n_out)]  # not monotonic
        nn, no = np.array(self.n, np.int32), np.array(self.n_out, np.int32)
        index = np.concatenate(self.index + [np.zeros(0, np.int32)])
        self.bad = np.zeros(3, np.int32)
        new = lib().rt_sim3_new if which else lib().rt_pnp_new
        smp = None if samples is None else np.ascontiguousarray(samples, np.int32)
        self.rc = new(self.K, p(nn), p(no), p(index), ctypes.addressof(params), S, p(smp), seed, p(self.bad))

    def info(self, c):
        o = np.zeros(10, np.int32)
        lib().rt_info(self.which, c, p(o))
        return dict(zip(["n", "n_out", "words", "min_inliers", "max_its", "alive", "iterations", "best_inliers", "best_row", "n_records"],
                        (int(v) for v in o)))

    def layout(self):
        off, words, mask_off, tot = [np.zeros(self.K, np.int32) for _ in range(3)] + [np.zeros(2, np.int64)]
        lib().rt_layout(self.which, p(off), p(words), p(mask_off), p(tot))
        return off, words, mask_off, int(tot[0]), int(tot[1])

    def load(self, pose, mask):
        """pose[c] (S, D) and mask[c] (S, n) bool per candidate, None for one without a solver: concatenated the way the
        device tables are (every candidate has its pose and count rows, only one with a solver has mask words)"""
        D = POSE[self.which]
        pose_all = np.concatenate([np.zeros((self.S, D)) if q is None else q for q in pose])
        count_all = np.concatenate([np.zeros(self.S, np.int32) if m is None else m.sum(axis=1).astype(np.int32) for m in mask])
        words = [pack(m).reshape(-1) for m in mask if m is not None]
        mask_all = np.concatenate(words + [np.zeros(0, np.uint64)])
        assert len(mask_all) == self.layout()[4]
        lib().rt_rows(self.which, p(np.ascontiguousarray(pose_all)), p(count_all), p(mask_all))

    def jobs(self):
        s = np.zeros(3, np.int64)
        lib().rt_pnp_sizes(p(s))
        jobs, idx = np.zeros((int(s[0]), 4), np.int32), np.zeros(int(s[1]), np.int32)
        lib().rt_pnp_jobs(p(jobs), p(idx))
        return jobs, idx, int(s[2])

    def iterate(self, c, n_iterations):
        found, n_inl, no_more, row = (ctypes.c_int32(-7) for _ in range(4))
        T = np.full(16, -7.0, np.float32)
        inliers = np.full(self.n_out[c], 0xFF, np.uint8)
        rc = lib().rt_iterate(self.which, c, n_iterations, ctypes.byref(found), p(T), p(inliers), ctypes.byref(n_inl),
                              ctypes.byref(no_more), ctypes.byref(row))
        return rc, found.value, no_more.value, n_inl.value, row.value, T, inliers

    def samples(self, c):
        """the sample rows alone (the tables of a handle may not be loaded yet)"""
        smp = np.full((self.S, 3 if self.which else 4), 0x5A, np.int32)
        assert lib().rt_tap_rows(self.which, c, p(smp), None, None, None) == VIEO_OK
        return smp

    def tap_rows(self, c, fill=0x5A):
        k, D, words = (3 if self.which else 4), POSE[self.which], (self.n[c] + 63) // 64
        smp = np.full((self.S, k), fill, np.int32)
        pose, count, mask = np.full((self.S, D), 7.5), np.full(self.S, fill, np.int32), np.full((self.S, words), fill, np.uint64)
        assert lib().rt_tap_rows(self.which, c, p(smp), p(pose), p(count), p(mask)) == VIEO_OK
        return smp, pose, count, mask


def same_result(got, want, T_want, n_out, where):
    """a call's outputs against the replay's result (PnPResult / Sim3Result)"""
    rc, found, no_more, n_inl, row, T, inliers = got
    assert rc == VIEO_OK and (found, no_more, n_inl, row) == (int(want.found), int(want.no_more), want.n_inliers, want.row), where
    if want.found:
        assert T.tobytes() == np.ascontiguousarray(T_want, np.float32).tobytes(), where
    else:
        assert (T == -7.0).all(), where  # not written
    vb = np.zeros(n_out, bool) if want.inliers is None else want.inliers
    assert np.array_equal(inliers, vb.astype(np.uint8)), where


# ---------------------------------------------------------------------------------------------------------------------
# the draw
M64 = (1 << 64) - 1


def splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw_restated(seed, cand, row, n, k):
    """splitmix64 of seed ^ (cand << 40), then + (row << 2) + i and mixed again; the pick is removed by swapping the
    last available index into its place"""
    avail, out = list(range(n)), []
    for i in range(k):
        r = splitmix64((splitmix64(seed ^ (cand << 40)) + (row << 2) + i) & M64)
        j = r % len(avail)
        out.append(avail[j])
        avail[j] = avail[-1]
        avail.pop()
    return out


def draw(seed, cand, row, n, k):
    out = np.full(k, -1, np.int32)
    lib().rt_draw(seed, cand, row, n, k, p(out))
    return out.tolist()


def test_the_draw_is_the_stated_generator():
    for seed in (0, 5, 0x123456789ABCDEF, M64):
        for cand in (0, 1, 7, 300):
            for row in (0, 1, 63, 511):
                for n, k in ((3, 3), (4, 3), (4, 4), (5, 4), (60, 3), (60, 4), (129, 4)):
                    assert draw(seed, cand, row, n, k) == draw_restated(seed, cand, row, n, k), (seed, cand, row, n, k)


def test_the_draw_is_the_parent_commits():
    """rows printed by pnp_draw of csrc/pnp.hip as it stood before the generator moved into ransac_table.h (commit
    71941a7), its text compiled as a stand-alone host program: (seed, cand, row, n, k) -> indices"""
    recorded = {(5, 0, 0, 60, 4): [9, 59, 33, 28], (5, 3, 63, 129, 4): [118, 18, 116, 89],
                (81985529216486895, 7, 511, 5, 4): [1, 3, 2, 0], (5, 0, 0, 60, 3): [9, 59, 33], (99, 2, 17, 4, 3): [3, 1, 0],
                (18446744073709551615, 15, 299, 300, 3): [216, 280, 281]}
    for args, want in recorded.items():
        assert draw(*args) == want, args


# ---------------------------------------------------------------------------------------------------------------------
# the sample filler
PNP_PARAMS = dict(probability=0.99, min_inliers=10, max_iterations=12, min_set=4, epsilon=0.5)
SIM3_PARAMS = dict(probability=0.99, min_inliers=20, max_iterations=300)


def pnp_params(**kw):
    q = dict(PNP_PARAMS, **kw)
    return PnpParams(q["probability"], q["min_inliers"], q["max_iterations"], q["min_set"], q["epsilon"], 5.991, 0)


def sim3_params(**kw):
    q = dict(SIM3_PARAMS, **kw)
    return Sim3Params(q["probability"], q["min_inliers"], q["max_iterations"])


@pytest.mark.parametrize("which", [PNP, SIM3])
def test_the_library_s_draw_fills_the_table(which):
    k = 3 if which else 4
    params = sim3_params(min_inliers=3) if which else pnp_params(min_inliers=4, epsilon=0.01)
    n = [k, k + 1, 0, 60, 60]  # the smallest sets, a candidate without a solver, two of one size
    tables = {}
    for seed in (5, 5, 6):
        H = Handle(which, n, params, 16, None, seed)
        assert H.rc == 0 and [H.info(c)["alive"] for c in range(5)] == [1, 1, 0, 1, 1]
        t = [H.samples(c) for c in range(5)]
        for c in (0, 1, 3, 4):
            assert ((t[c] >= 0) & (t[c] < n[c])).all() and all(len(set(r)) == k for r in t[c].tolist()), (seed, c)
            assert t[c].tolist() == [draw(seed, c, r, n[c], k) for r in range(16)]
        assert (t[2] == 0).all()  # no solver: the rows stay zero
        assert len({tuple(r) for r in t[3].tolist()}) > 8 and not np.array_equal(t[3], t[4])  # rows differ, candidates differ
        if seed in tables:
            assert all(np.array_equal(a, b) for a, b in zip(tables[seed], t))
        tables[seed] = t
    assert not np.array_equal(tables[5][3], tables[6][3])


@pytest.mark.parametrize("which", [PNP, SIM3])
def test_a_caller_s_table_is_checked(which):
    k = 3 if which else 4
    params = sim3_params(min_inliers=3) if which else pnp_params(min_inliers=4, epsilon=0.01)
    n, S = [9, 2, 12], 6  # candidate 1 has no solver: its rows are not looked at
    good = np.stack([np.stack([np.random.default_rng([c, r]).permutation(max(n[c], k))[:k] for r in range(S)]) for c in range(3)])
    good[1] = 99
    H = Handle(which, n, params, S, good)
    assert H.rc == 0 and np.array_equal(H.samples(0), good[0]) and np.array_equal(H.samples(2), good[2])
    assert (H.samples(1) == 0).all()
    for (c, r, i), value in {(0, 2, 1): 9, (2, 5, k - 1): 12, (2, 0, 0): -1, (0, 4, 2): None, (2, 3, k - 1): None}.items():
        t = good.copy()
        t[c, r, i] = t[c, r, 0] if value is None else value  # None: an index of the row a second time
        H = Handle(which, n, params, S, t)
        assert H.rc == -1 and H.bad.tolist() == [c, r, int(t[c, r, i])], (c, r, i, H.bad)


def test_the_iteration_count():
    """ceil(log(1 - p) / log(1 - eps^3)) inside [1, max_iterations]; the cases that are no number: eps = 0 gives -inf
    (1), eps = 1 gives 0 (1), p = 1 gives +inf and p > 1 a NaN (both the cap); min_inliers == N is 1 whatever the rest"""
    f = lib().rt_max_iterations
    for prob, eps, cap in ((0.99, 0.5, 300), (0.99, 0.5, 20), (0.99, 0.3125, 300), (0.999, 0.1, 100000), (0.5, 0.9, 300)):
        want = max(1, min(int(np.ceil(np.log(1 - prob) / np.log(1 - float(np.float32(eps)) ** 3))), cap))
        assert f(prob, eps, 10, 60, cap) == want
    assert f(0.99, 0.5, 10, 60, 300) == 35
    assert [f(0.99, 0.0, 10, 60, 300), f(0.99, 1.0, 10, 60, 300), f(1.0, 0.5, 10, 60, 300), f(1.5, 0.5, 10, 60, 300)] == [1, 1, 300, 300]
    assert f(0.99, 0.5, 60, 60, 300) == 1 and f(1.5, 0.0, 60, 60, 300) == 1
    for N in (20, 21, 33, 64, 129, 1000):  # both solvers' parameters against the restatements'
        H = Handle(PNP, [N], pnp_params(max_iterations=300), 1)
        assert (H.info(0)["min_inliers"], H.info(0)["max_its"]) == reloc_ref.ransac_parameters(N, **dict(PNP_PARAMS, max_iterations=300))
        H = Handle(SIM3, [N], sim3_params(), 1)
        assert (H.info(0)["min_inliers"], H.info(0)["max_its"]) == loop_ref.ransac_parameters(N, **SIM3_PARAMS)


# ---------------------------------------------------------------------------------------------------------------------
# PnPsolver::iterate over the two tables
def pnp_case(rng, n, S, deltas, rec_deltas):
    """counts = mRansacMinInliers + deltas for the first rows, random ones after them; rec_deltas likewise for the records
    in the order they open.  mRansacMinInliers = n / 2 (epsilon 0.5)."""
    m = n // 2
    deltas = list(deltas) + rng.integers(-10, min(26, n - m + 1), max(S - len(deltas), 0)).tolist()
    count = np.clip(m + np.array(deltas[:S]), 0, n)
    return dict(n=n, m=m, pose=rng.standard_normal((S, 12)), mask=masks_with(rng, n, count), count=count, rec_deltas=list(rec_deltas))


def pnp_handle(S, seed):
    rng = np.random.default_rng(seed)
    opening = [-12, 0, 0, -22, 8, 4, 1, 13, 2, -1, 13, 20, 3]  # records at rows 1, 4, 7, 11; rows 5 and 6 answer with 4's
    cases = [pnp_case(rng, 64, S, opening, [0, 9, -2, 1]), None, pnp_case(rng, 129, S, [1, -30, 3, 2, 3, -1, 5] + [-2] * 40, [-1, 0, -5]),
             None, pnp_case(rng, 65, S, [-1, -5, -32, -2] * 12, []), None, pnp_case(rng, 65, S, opening, [0, 9, -2, 1])]
    n = [c["n"] if c else d for c, d in zip(cases, (0, 0, 0, 3, 0, 8, 0))]  # no solver: n = 0, 3 and 4 <= n < mRansacMinInliers
    H = Handle(PNP, n, pnp_params(), S, rng=rng)
    assert H.rc == 0
    H.load([c and c["pose"] for c in cases], [c and c["mask"] for c in cases])
    return H, cases, rng


def records_by_numpy(count, m):
    """the rows that raise the best-so-far set: count >= mRansacMinInliers and above every earlier such count"""
    ok = np.where(count >= m, count, 0)
    return np.flatnonzero((ok > 0) & (ok > np.concatenate([[0], np.maximum.accumulate(ok)[:-1]])))


@pytest.mark.parametrize("S", [40, 8])
def test_pnp_records_and_iterate(S):
    H, cases, rng = pnp_handle(S, 11)
    # ---- the layout and the records
    off, words, mask_off, n_all, words_all = H.layout()
    alive = [c is not None for c in cases]
    assert off.tolist() == np.concatenate([[0], np.cumsum(H.n)[:-1]]).tolist() and n_all == sum(H.n)
    assert words.tolist() == [(k + 63) // 64 if a else 0 for k, a in zip(H.n, alive)]
    assert mask_off.tolist() == np.concatenate([[0], np.cumsum(words * S)[:-1]]).tolist() and words_all == int((words * S).sum())
    jobs, idx, rec_words = H.jobs()
    want_jobs, want_idx, w = [], [], 0
    for c, q in enumerate(cases):
        q = q or dict(count=np.zeros(S, int), m=1)
        q["rec_row"] = records_by_numpy(q["count"], q["m"])
        for r in q["rec_row"]:
            want_jobs.append([c, len(want_idx), q["count"][r], w])
            want_idx += np.flatnonzero(q["mask"][r]).tolist()
            w += int(words[c])
        assert H.info(c)["n_records"] == len(q["rec_row"])
    assert jobs.tolist() == want_jobs and idx.tolist() == want_idx and rec_words == w and len(want_jobs) > 6
    assert cases[0]["rec_row"][:4].tolist() == [1, 4, 7, 11][:len(cases[0]["rec_row"][:4])]
    # ---- pass B's tables: per job a pose, a count around mRansacMinInliers and a mask of that count
    rec_Rt, rec_count, rec_mask = rng.standard_normal((len(jobs), 12)), np.zeros(len(jobs), np.int32), []
    for j, (c, _, _, _) in enumerate(jobs.tolist()):
        d = cases[c]["rec_deltas"]
        k = len([1 for jj in range(j) if jobs[jj, 0] == c])
        rec_count[j] = cases[c]["m"] + (d[k] if k < len(d) else int(rng.integers(-3, 6)))
        rec_mask.append(masks_with(rng, cases[c]["n"], [rec_count[j]]))
    lib().rt_pnp_records(p(rec_Rt), p(rec_count), p(np.concatenate([pack(m).reshape(-1) for m in rec_mask])))
    # ---- the rows come back as they went in; a candidate without a solver has rows of zeros
    for c, q in enumerate(cases):
        smp, pose, count, mask = H.tap_rows(c)
        if q is None:
            assert not smp.any() and not pose.any() and not count.any() and not mask.any()
        else:
            assert np.array_equal(pose, q["pose"]) and np.array_equal(count, q["count"]) and np.array_equal(mask, pack(q["mask"]))
    # ---- iterate(5), call by call, against the replay
    seen = dict(exact=0, earlier_record=0, best_at_no_more=0, nothing=0, capacity=0, dead=0)
    for c, q in enumerate(cases):
        info = H.info(c)
        if q is None:
            replay = reloc_ref.IterateReplay((np.zeros((S, 12)), np.zeros(S, int), np.zeros((S, H.n[c]), bool)), ([], [], [], []),
                                             info["min_inliers"], info["max_its"], H.index[c], H.n_out[c])
            for call in range(2):
                want = replay.iterate(5)
                assert want.no_more and not want.found
                same_result(H.iterate(c, 5), want, None, H.n_out[c], (c, call))
                assert (H.info(c)["iterations"], H.info(c)["best_row"]) == (0, -1)
            seen["dead"] += 1
            continue
        assert (info["min_inliers"], info["max_its"]) == reloc_ref.ransac_parameters(q["n"], **PNP_PARAMS) == (q["m"], 12)
        mine = [j for j in range(len(jobs)) if jobs[j, 0] == c]
        records = (q["rec_row"], rec_Rt[mine], rec_count[mine], np.concatenate([rec_mask[j] for j in mine] + [np.zeros((0, q["n"]), bool)]))
        replay = reloc_ref.IterateReplay((q["pose"], q["count"], q["mask"]), records, q["m"], 12, H.index[c], H.n_out[c])
        for call in range(S + 1):  # (a call that does not end at the table's end takes a row at least)
            first = replay.iterations
            want, got = replay.iterate(5), H.iterate(c, 5)
            now = H.info(c)
            assert (now["iterations"], now["best_inliers"], now["best_row"]) == (replay.iterations, replay.best_inliers, replay.best_row)
            if want.no_more == 2:  # the replay's sign for a row beyond the table
                assert got[0] == VIEO_E_CAPACITY and got[1:5] == (0, 0, 0, -1) and not got[6].any(), (c, call)
                assert lib().rt_error().decode() == "PnPsolver: candidate %d needs sample row %d, the table has %d" % (c, S, S)
                seen["capacity"] += 1
                break
            same_result(got, want, want.Tcw, H.n_out[c], (c, call))
            for r in range(first, replay.iterations):  # a row of exactly mRansacMinInliers became the best and was not returned
                seen["exact"] += q["count"][r] == q["m"] and r in q["rec_row"] and not (want.found and want.row == r)
            if want.found and not want.no_more:
                seen["earlier_record"] += q["count"][want.row] < replay.best_inliers
                assert want.n_inliers > q["m"]
            if want.found and want.no_more:
                assert want.n_inliers == replay.best_inliers and want.row == replay.best_row
                assert got[5].tobytes() == reloc_ref.tcw_float(q["pose"][want.row][:9].reshape(3, 3), q["pose"][want.row][9:]).tobytes()
                planted = [b for b in PLANTED if b < q["n"]]
                assert got[6][H.index[c][planted]].all() and got[6].sum() == want.n_inliers
                seen["best_at_no_more"] += len(planted) == 4  # the candidate of 129: three mask words
            seen["nothing"] += bool(want.no_more and not want.found and replay.best_inliers < q["m"])
    assert seen["dead"] == 3 and seen["capacity"] == 4, seen  # S = 8: n_rows < mRansacMaxIts; S = 40: rows used up after bNoMore
    if S == 40:  # (with 8 rows every candidate runs out of rows before mRansacMaxIts = 12)
        assert seen["best_at_no_more"] > 0 and seen["nothing"] > 0 and seen["exact"] > 0 and seen["earlier_record"] > 0, seen


# ---------------------------------------------------------------------------------------------------------------------
# Sim3Solver::iterate over the table
def sim3_case(rng, n, S, counts):
    count = np.array(list(counts) + rng.integers(0, min(n, 40) + 1, S).tolist())[:S]
    return dict(n=n, pose=rng.standard_normal((S, 13)), mask=masks_with(rng, n, count), count=count)


@pytest.mark.parametrize("max_iterations, S", [(300, 40), (23, 40), (300, 12)])
def test_sim3_iterate_and_estimate(max_iterations, S):
    rng = np.random.default_rng(12)
    m = SIM3_PARAMS["min_inliers"]
    opening = [15, 15, m, 18, m, 25, 19, 25, 24, 30, 30, 12]  # ties at rows 1, 4, 7, 10; row 2 is exactly mRansacMinInliers
    cases = [sim3_case(rng, 64, S, opening), None, sim3_case(rng, 65, S, opening[::-1]), sim3_case(rng, 129, S, [4, 4, m, m + 1, 70])]
    n = [c["n"] if c else 10 for c in cases]
    H = Handle(SIM3, n, sim3_params(max_iterations=max_iterations), S, rng=rng)
    assert H.rc == 0
    H.load([c and c["pose"] for c in cases], [c and c["mask"] for c in cases])
    params = dict(SIM3_PARAMS, max_iterations=max_iterations)
    seen = dict(tie=0, exact=0, stopped_after_n=0, capacity=0, no_more=0, dead=0)
    R, t, s = np.zeros(9, np.float32), np.zeros(3, np.float32), ctypes.c_float(0)
    for c, q in enumerate(cases):
        cand = dict(X1=np.zeros((n[c], 3)), n1=H.n_out[c], index1=H.index[c])
        tables = (q["pose"], q["mask"]) if q else (np.zeros((S, 13)), np.zeros((S, n[c]), bool))
        replay = loop_ref.Sim3SolverRef(cand, np.zeros((S, 3), int), params, tables=tables)
        assert (H.info(c)["min_inliers"], H.info(c)["max_its"]) == (replay.min_inliers, replay.max_its)
        assert lib().rt_sim3_estimate(c, p(R), p(t), ctypes.byref(s)) == VIEO_E_EMPTY and replay.estimate() is None
        assert lib().rt_error().decode() == "Sim3Solver: candidate %d has no estimate yet" % c
        if q is None:
            want = replay.iterate(5)
            assert want.no_more and not want.found
            same_result(H.iterate(c, 5), want, None, H.n_out[c], c)
            assert lib().rt_sim3_estimate(c, p(R), p(t), ctypes.byref(s)) == VIEO_E_EMPTY
            smp, pose, count, mask = H.tap_rows(c)
            assert not smp.any() and not pose.any() and not count.any() and not mask.any()
            seen["dead"] += 1
            continue
        _, pose, count, mask = H.tap_rows(c)
        assert np.array_equal(pose, q["pose"]) and np.array_equal(count, q["count"]) and np.array_equal(mask, pack(q["mask"]))
        for call in range(12):
            first = replay.iterations
            want, got = replay.iterate(5), H.iterate(c, 5)
            now = H.info(c)
            assert (now["iterations"], now["best_inliers"], now["best_row"]) == (replay.iterations, replay.best_inliers, replay.best_row)
            if want.no_more == 2:
                assert got[0] == VIEO_E_CAPACITY and got[1:5] == (0, 0, 0, -1) and not got[6].any(), (c, call)
                assert lib().rt_error().decode() == "Sim3Solver: candidate %d needs sample row %d, the table has %d" % (c, S, S)
                seen["capacity"] += 1
                break
            same_result(got, want, want.T12, H.n_out[c], (c, call))
            if want.found:
                planted = [b for b in PLANTED if b < q["n"]]
                assert want.n_inliers > m and got[6][H.index[c][planted]].all() and got[6].sum() == want.n_inliers
            assert lib().rt_sim3_estimate(c, p(R), p(t), ctypes.byref(s)) == VIEO_OK
            for x, y in zip((R.reshape(3, 3), t, np.float32(s.value)), replay.estimate()):
                assert np.asarray(x).tobytes() == np.asarray(y, np.float32).tobytes()
            for r in range(first, replay.iterations):
                seen["tie"] += r > 0 and q["count"][r] == q["count"][:r].max() and replay.best_row >= r
                seen["exact"] += q["count"][r] == m and q["count"][r] >= q["count"][:r + 1].max() and not (want.found and want.row == r)
            seen["stopped_after_n"] += not want.found and not want.no_more and replay.iterations - first == 5
            if want.no_more:
                seen["no_more"] += 1
                assert replay.iterations == replay.max_its == 23
                break
    assert seen["dead"] == 1 and seen["tie"] > 0 and seen["exact"] > 0 and seen["stopped_after_n"] > 0, seen
    assert (seen["no_more"], seen["capacity"]) == ((3, 0) if max_iterations == 23 else (0, 3)), seen


def test_mark_inliers_through_the_index_map():
    """the mask words of n = 64, 65 and 129 correspondences, bits 0, 63, 64 and 128 among them, into n + 37 entries"""
    rng = np.random.default_rng(3)
    for n in (64, 65, 129):
        index = rng.permutation(n + 37)[:n].astype(np.int32)
        assert (np.diff(index) < 0).any()
        for k in (len([b for b in PLANTED if b < n]), 20, n):
            mask = masks_with(rng, n, [k])
            out = np.zeros(n + 37, np.uint8)
            lib().rt_mark_inliers(p(pack(mask)), n, p(index), p(out))
            want = np.zeros(n + 37, np.uint8)
            want[index[mask[0]]] = 1
            assert np.array_equal(out, want) and out.sum() == k and out[index[[b for b in PLANTED if b < n]]].all()
