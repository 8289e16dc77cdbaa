"""Planted inputs for Frame::ComputeStereoMatches (tests/test_stereo_ref.py on the host, tests/test_stereo_edges.py on the
device).  Test infrastructure only.

Both entry points of the stereo stage and the oracle take caller-supplied keys and descriptors and read only the
pyramids from the extractors, so a case is a frame: an image pair, keys and descriptors planted on it, and a `check`
that asserts from the census of tests/stereo_ref.py that the frame reaches the branches it is named for.

How the values are controlled (octave 0, where the plane is the input image):
  descriptors  a right row is a left row with k chosen bits flipped: the distance is k.
  SADs         `paint` writes a random 11 x 21 strip around a right key and its window at increment e as the 11 x 11
               patch around the left key: the SAD at e is 0, every other one large, bestincR = e.  Adding v to the
               top-left pixel of that window makes the best SAD exactly v.  Keys sit at least 32 columns or 11 rows
               apart, so strips do not overlap.
  deltaR       a strip that is mirror-symmetric about its centre column gives dist1 == dist3, deltaR = 0 exactly; rows
               that are constant over twelve columns give SAD 0 at two increments, the first wins, dist2 == dist3 and
               deltaR = +0.5.  (-0.5 would need dist1 == dist2, but then the earlier increment is the best one; and
               |deltaR| > 1 needs 4 dist2 > dist1 + 3 dist3 with dist2 the minimum: the deltaR gate cannot close on
               finite values.  A 0 / 0 gives NaN, which passes that gate and ends at the disparity gate.)
All frames use bf = 20, baseline = 1: maxD = 20 px, so that the disparity gates are reachable on a small frame.

The domain (asserted in Frame.add_left, and in Frame.assert_domain on the census): 0 <= (int)y < rows for a left key and its 11 x 11 patch
inside its level -- unless x < 0, which ends at maxU < 0 before anything is read; a right key that passes a left key's
gates has round(xR * inv_L) >= 10 at the left key's level (below that the reference's colRange starts negative: the
kernel clamps, the oracle reads outside its plane); octaves 0..7.
"""
import numpy as np

from tests import stereo_ref
from tests.oracle_lib import KEYPOINT_DTYPE
from vieo_slam_amd import synth

BF, BASELINE, MAXD = 20.0, 1.0, 20.0
NLEVELS, SCALE = 8, np.float32(1.2)
f32 = np.float32


def scale_factors():
    """mvScaleFactor / mvInvScaleFactor as the extractors build them (float products, float reciprocals)."""
    s = np.ones(NLEVELS, np.float32)
    for l in range(1, NLEVELS):
        s[l] = f32(s[l - 1] * SCALE)
    return s, (f32(1.0) / s).astype(np.float32)


def level_sizes(w, h):
    _, inv = scale_factors()
    return [(int(np.rint(f32(f32(w) * inv[l]))), int(np.rint(f32(f32(h) * inv[l])))) for l in range(NLEVELS)]


def base_pair(w, h, seed=4000):
    """two unrelated textured images (the extractors' usual synthetic frames)"""
    return synth.synth_image(seed, w, h), synth.synth_image(seed + 1, w, h)


class Frame:
    def __init__(self, name, w, h, seed=0):
        self.name, self.w, self.h = name, w, h
        self.left, self.right = (a.copy() for a in _BASE.setdefault((w, h), base_pair(w, h)))
        self.rng = np.random.default_rng(seed + 17)
        self.kl, self.dl, self.kr, self.dr = [], [], [], []
        self.tags = {}
        self.checks = []
        self.scale, self.inv = scale_factors()
        self.sizes = level_sizes(w, h)

    # ---- keys
    def rand_desc(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    @staticmethod
    def flip(desc, k, first=0):
        bits = np.unpackbits(desc)
        bits[first:first + k] ^= 1
        return np.packbits(bits)

    def add_left(self, x, y, octave=0, desc=None, tag=None):
        x, y = f32(x), f32(y)
        assert 0 <= octave < NLEVELS and 0 <= int(y) < self.h
        if not x < 0:
            lw, lh = self.sizes[octave]
            su, sv = stereo_ref.c_round(f32(x * self.inv[octave])), stereo_ref.c_round(f32(y * self.inv[octave]))
            assert su - 5 >= 0 and su + 5 < lw and sv - 5 >= 0 and sv + 5 < lh, "left patch outside its level"
        self.kl.append((x, y, 31.0, 0.0, 50.0, octave, -1))
        self.dl.append(self.rand_desc() if desc is None else desc)
        if tag is not None:
            self.tags[tag] = len(self.kl) - 1
        return len(self.kl) - 1

    def add_right(self, x, y, octave=0, desc=None):
        assert 0 <= octave < NLEVELS
        self.kr.append((f32(x), f32(y), 31.0, 0.0, 50.0, octave, -1))
        self.dr.append(self.rand_desc() if desc is None else desc)
        return len(self.kr) - 1

    # ---- pixels (octave 0)
    def paint(self, ul, ur, y, e=0, sad=0, kind="random"):
        cl, cr, r = int(stereo_ref.c_round(ul)), int(stereo_ref.c_round(ur)), int(stereo_ref.c_round(y))
        assert r - 5 >= 0 and r + 5 < self.h and cl - 5 >= 0 and cl + 5 < self.w and cr - 10 >= 0 and cr + 10 < self.w
        strip = self.rng.integers(40, 200, (11, 21)).astype(np.uint8)
        if kind == "symmetric":
            strip[:, 11:] = strip[:, 9::-1]
        elif kind == "two_minima":  # windows e and e + 1 are equal
            strip[:, 5 + e:17 + e] = strip[:, 5 + e:6 + e]
        elif kind == "near_minus":  # windows e - 1 and e are equal but for one pixel: dist1 = dist2 + 1
            strip[:, 4 + e:16 + e] = strip[:, 4 + e:5 + e]
            strip[0, 4 + e] += 1
        elif kind == "flat":
            strip[:] = 90
        elif kind == "checker":
            strip[:] = (255 * ((np.add.outer(np.arange(11), np.arange(21)) + 1) % 2)).astype(np.uint8)
        elif kind == "extreme":  # left: white, black centre; right window e: black, white centre.  SAD(e) = 120 * 510
            strip[:] = 0
            strip[5, 10 + e] = 255
        patch = strip[:, 5 + e:16 + e].copy()
        if kind == "checker":
            patch = 255 - patch  # the opposite phase: |il - ir| = 510 on 60 pixels
        elif kind == "extreme":
            patch[:] = 255
            patch[5, 5] = 0
        if sad and kind == "symmetric":  # half of it on either side of the centre column: still symmetric
            assert sad % 2 == 0 and e == 0
            strip[0, 5] += sad // 2
            strip[0, 15] += sad // 2
        elif sad:
            assert kind == "random"
            strip[0, 5 + e] += sad
        self.right[r - 5:r + 6, cr - 10:cr + 11] = strip
        self.left[r - 5:r + 6, cl - 5:cl + 6] = patch

    def pair(self, ul, y, ur, e=0, sad=0, k=0, kind="random", tag=None):
        """a left key, its right key at distance k and the pixels that make bestincR = e with best SAD `sad`"""
        d = self.rand_desc()
        self.paint(ul, ur, y, e, sad, kind)
        il = self.add_left(ul, y, 0, d, tag)
        return il, self.add_right(ur, y, 0, self.flip(d, k))

    def ballast(self, n, y, sad=8):
        """n accepted matches of SAD `sad` on row y: they keep the frame's median above 0, so that its accepted matches
        of SAD 0 survive the median rejection and show in the output"""
        for i in range(n):
            self.pair(30.0 + 34 * i, y, 21.0 + 34 * i, sad=sad, tag="ballast%d" % i)
            self.expect("ballast%d" % i, gate="accepted", sad=sad)

    def expect(self, tag, **want):
        """census fields of the tagged left key that the frame promises"""
        self.checks.append((tag, want))

    # ---- the finished frame
    def finish(self):
        self.kl = np.array(self.kl, KEYPOINT_DTYPE) if self.kl else np.zeros(0, KEYPOINT_DTYPE)
        self.kr = np.array(self.kr, KEYPOINT_DTYPE) if self.kr else np.zeros(0, KEYPOINT_DTYPE)
        self.dl = np.array(self.dl, np.uint8).reshape(-1, 32)
        self.dr = np.array(self.dr, np.uint8).reshape(-1, 32)
        return self

    def assert_domain(self, census):
        """every right key that passed a left key's gates and could be refined starts its strip inside the plane"""
        for i, rec in enumerate(census):
            if rec["best_idx"] >= 0 and rec["best_dist"] < 75:
                lv = int(self.kl["octave"][i])
                assert stereo_ref.c_round(f32(self.kr["x"][rec["best_idx"]] * self.inv[lv])) >= 10, (self.name, i)

    def check(self, census):
        self.assert_domain(census)
        for tag, want in self.checks:
            rec = census[self.tags[tag]]
            for key, val in want.items():
                if key == "frame":  # a property of the whole frame
                    assert val(census), (self.name, tag)
                elif callable(val):
                    assert val(rec[key]), (self.name, tag, key, rec[key])
                else:
                    assert rec[key] == val, (self.name, tag, key, rec[key], val)


_BASE = {}


# ------------------------------------------------------------------ the frames
def frame_rows(w, h):
    """the row table: bands clipped at row 0 and rows - 1, an integer y, a 16-row octave-7 band, an empty row"""
    F = Frame("rows", w, h, 1)
    d = F.rand_desc()
    # a band clipped at row 0: y = 2, r = 2: rows floor(0) .. ceil(4) at octave 0; at octave 1 r = 2.4: -1 .. 5
    F.add_right(100, 2.0, 1, d)
    F.add_left(108, 5.0, 0, F.flip(d, 3), "clip0")
    F.add_left(140, 6.0, 0, F.flip(d, 3), "clip0_below")
    F.expect("clip0", row=5, n_cand=1, n_gated=1)
    F.expect("clip0_below", row=6, n_cand=0, gate="no_candidate")
    # a band clipped at the last row: y = h - 3, r = 2.4: rows h - 6 .. h (clipped to h - 1)
    d = F.rand_desc()
    F.add_right(100, h - 3.0, 1, d)
    F.add_left(108, h - 6 + 0.4, 0, F.flip(d, 3), "clipH")  # the last row a patch of octave 0 fits in
    F.expect("clipH", row=h - 6, n_cand=1, n_gated=1)
    # an integer y: floor = ceil, rows 38 .. 42
    d = F.rand_desc()
    F.add_right(100, 40.0, 0, d)
    for x, y, n in ((108, 37.0, 0), (140, 38.0, 1), (172, 42.0, 1), (204, 43.0, 0), (76, 42.99, 1)):
        F.add_left(x, y, 0, F.flip(d, 2), "int%d_%g" % (x, y))
        F.expect("int%d_%g" % (x, y), row=int(y), n_cand=n)
    # octave 7: r = 2 * 1.2^7 = 7.17, y = 100.3: rows 93 .. 108, sixteen of them
    d = F.rand_desc()
    F.add_right(120, 100.3, 7, d)
    for x, y, n in ((122, 92.0, 0), (126, 93.0, 1), (130, 108.5, 1), (134, 109.0, 0)):
        F.add_left(x, y, 6, F.flip(d, 2), "oct7_%g" % y)
        F.expect("oct7_%g" % y, row=int(y), n_cand=n, n_gated=n)
    # x < 0: ends at maxU < 0 although its row has a candidate
    d = F.rand_desc()
    F.add_right(30, 150.0, 0, d)
    F.add_left(-1.0, 150.0, 0, d, "negx")
    F.expect("negx", n_cand=1, gate="maxU<0")
    return F.finish()


def _stack(F, y, n, winner_pos, tag, ul=150.0, k_win=5, sad=8):
    """n right keys on row y, all inside [uL - maxD, uL]; the one at position `winner_pos` of the row matches"""
    d = F.rand_desc()
    first = len(F.kr)
    win_x = f32(ul - 8)
    for j in range(n):
        if j == winner_pos:
            F.add_right(win_x, y, 0, F.flip(d, k_win))
        else:  # competitive losers: distance 20 .. 59, x anywhere inside the gate
            F.add_right(f32(ul - 19.5 + 19.0 * j / max(n - 1, 1)), y, 0, F.flip(d, 20 + (j * 7) % 40, 64))
    F.paint(ul, win_x, y, sad=sad)
    F.add_left(ul, y, 0, d, tag)
    F.expect(tag, n_cand=n, n_gated=n, best_idx=first + winner_pos, best_dist=k_win, gate="accepted", best_inc=0, sad=sad)


def frame_counts(w, h):
    """rows with exactly 1, 16, 17, 32, 33, 64 and 65 candidates, the winner the last key of its row"""
    F = Frame("counts", w, h, 2)
    for i, n in enumerate((1, 16, 17, 32, 33, 64, 65)):
        _stack(F, 20.0 + 30 * i, n, n - 1, "n%d" % n, sad=8 + i)
    return F.finish()


def frame_counts_first(w, h):
    """the same rows with the winner first, and in the middle of the second pass"""
    F = Frame("counts_first", w, h, 3)
    for i, (n, pos) in enumerate(((16, 0), (17, 16), (33, 0), (33, 32), (64, 40), (65, 0), (65, 33))):
        _stack(F, 20.0 + 30 * i, n, pos, "n%d_p%d" % (n, pos), ul=100.0 + 10 * i, sad=8 + i)
    return F.finish()


def frame_ties(w, h):
    """equal best distances: the lower right index wins, whichever lane or pass holds it"""
    F = Frame("ties", w, h, 4)
    for i, (n, lo, hi) in enumerate(((2, 0, 1), (40, 3, 37), (40, 19, 20), (65, 0, 64), (65, 31, 32), (20, 2, 18))):
        y, ul = 20.0 + 30 * i, 150.0
        d = F.rand_desc()
        first = len(F.kr)
        for j in range(n):
            if j == lo:
                F.add_right(ul - 6, y, 0, F.flip(d, 10, 0))
            elif j == hi:
                F.add_right(ul - 15, y, 0, F.flip(d, 10, 100))  # the same distance through other bits, another column
            else:
                F.add_right(f32(ul - 19.5 + 19.0 * j / (n - 1)), y, 0, F.flip(d, 30 + j % 30, 30))
        F.paint(ul, ul - 6, y, sad=8 + i)
        tag = "tie%d_%d_%d" % (n, lo, hi)
        F.add_left(ul, y, 0, d, tag)
        F.expect(tag, n_cand=n, best_dist=10, best_idx=first + lo, tied=[first + lo, first + hi], gate="accepted")
    # a tie where the higher index would have been refined and the lower one is rejected at +L
    y, ul = 20.0 + 30 * 6, 150.0
    d = F.rand_desc()
    first = len(F.kr)
    F.add_right(ul - 13, y, 0, F.flip(d, 4, 0))
    F.add_right(ul - 8, y, 0, F.flip(d, 4, 50))
    F.paint(ul, ul - 8, y)
    F.add_left(ul, y, 0, d, "tie_reject")
    F.expect("tie_reject", tied=[first, first + 1], best_idx=first, gate="bestincR=+L")
    return F.finish()


def frame_tie_order(w, h):
    """ties whose lowest index comes late in the row's list.  The kernels build a row's list with atomic cursors, a
    thread per right key walking its band from the top: a key whose band ENDS at row Y gets there rounds after the keys
    whose bands BEGIN at Y, so the lowest index (octave 1, band Y - 5 .. Y) stands behind the others (octave 0, bands
    Y .. Y + 4) -- with 17 or 33 candidates in the very lane of the search that holds the list's first entry.  All
    candidates are at the same distance: whatever the order, the lowest index must win."""
    F = Frame("tie_order", w, h, 8)
    for i, n in enumerate((17, 33, 2, 49)):
        Y, ul = 30 + 45 * i, 150.0
        d = F.rand_desc()
        first = len(F.kr)
        F.add_right(ul - 6, Y - 2.5, 1, F.flip(d, 10, 0))
        for j in range(1, n):
            F.add_right(f32(ul - 19.5 + 8.0 * j / n), Y + 2.0, 0, F.flip(d, 10, 20 + j))
        F.paint(ul, ul - 6, Y + 0.4, sad=8 + i)
        tag = "order%d" % n
        F.add_left(ul, Y + 0.4, 0, d, tag)
        F.expect(tag, row=Y, n_cand=n, n_gated=n, best_dist=10, best_idx=first, tied=list(range(first, first + n)),
                 gate="accepted", sad=8 + i)
    return F.finish()


def frame_gates(w, h):
    """octave gate, the [minU, maxU] gate at its ends, the distance thresholds"""
    F = Frame("gates", w, h, 5)
    y = 12.0
    # a closer candidate two octaves off loses to a farther one at the same octave
    d = F.rand_desc()
    F.add_right(100, y, 2, d)
    b = F.add_right(100, y, 0, F.flip(d, 20))
    F.paint(110, 100, y, sad=8)
    F.add_left(110, y, 0, d, "two_octaves")
    F.expect("two_octaves", n_cand=2, n_gated=1, best_idx=b, best_dist=20)
    # left octave 0 against right octaves 0, 1, 2
    for o, g in ((0, 1), (1, 1), (2, 0)):
        y += 16
        d = F.rand_desc()
        F.add_right(60, y, o, d)
        F.add_left(70, y, 0, F.flip(d, 1), "L0_R%d" % o)
        F.expect("L0_R%d" % o, n_gated=g, gate=(lambda v: v != "bestDist>=75") if g else "bestDist>=75")
    # uR == uL and uR == uL - maxD are inside, one ulp beyond is outside
    ul = f32(120.0)
    for tag, ur, g in (("u_eq_max", ul, 1), ("u_above_max", np.nextafter(ul, f32(1e9)), 0),
                       ("u_eq_min", f32(100.0), 1), ("u_below_min", np.nextafter(f32(100.0), f32(-1e9)), 0)):
        y += 16
        d = F.rand_desc()
        F.paint(ul, ur, y, sad=8, kind="symmetric")
        F.add_right(ur, y, 0, d)
        F.add_left(ul, y, 0, d, tag)
        F.expect(tag, n_cand=1, n_gated=g)
    F.expect("u_eq_max", gate="accepted", zero_branch=True, delta_r=0)  # disparity exactly 0: the 0.01 branch
    F.expect("u_eq_min", gate="disparity", delta_r=0)                    # disparity exactly maxD: outside
    # just below maxD
    y += 16
    d = F.rand_desc()
    ulb = np.nextafter(f32(120.0), f32(0))
    F.paint(ulb, 100.0, y, sad=8, kind="symmetric")
    F.add_right(100.0, y, 0, d)
    F.add_left(ulb, y, 0, d, "below_maxD")
    F.expect("below_maxD", gate="accepted", delta_r=0, zero_branch=False)
    # best distance 74, 75, 99, 100
    for i, k in enumerate((74, 75, 99, 100)):
        yy = 150.0 + 16 * i
        d = F.rand_desc()
        F.paint(50, 42, yy, sad=8)
        F.add_right(42, yy, 0, F.flip(d, k))
        F.add_left(50, yy, 0, d, "dist%d" % k)
    F.expect("dist74", best_dist=74, gate="accepted")
    F.expect("dist75", best_dist=75, best_idx=lambda j: j >= 0, gate="bestDist>=75")
    F.expect("dist99", best_dist=99, best_idx=lambda j: j >= 0, gate="bestDist>=75")
    F.expect("dist100", best_dist=100, best_idx=-1, gate="bestDist>=75")
    return F.finish()


def frame_oct7(w, h):
    """left octave 7 against right octaves 5, 6, 7 (bands of 11 to 16 rows)"""
    F = Frame("oct7", w, h, 7)
    for i, (o, g) in enumerate(((5, 0), (6, 1), (7, 1))):
        yy = 40.0 + 50 * i
        d = F.rand_desc()
        F.add_right(160, yy, o, d)
        F.add_left(175, yy, 7, F.flip(d, 1), "L7_R%d" % o)
        F.expect("L7_R%d" % o, n_cand=1, n_gated=g, gate=(lambda v: v != "bestDist>=75") if g else "bestDist>=75")
    return F.finish()


def _x_for_scaled(F, octave, target):
    """a float x with round(x * inv[octave]) == target"""
    x = f32(f32(target) * F.scale[octave])
    assert stereo_ref.c_round(f32(x * F.inv[octave])) == target
    return x


def frame_refine(w, h):
    """the refinement: the endu gate at both octaves, bestincR at its ends, equal SADs, flat, largest sums"""
    F = Frame("refine", w, h, 6)
    y = 10.0
    # round(uR0) + 11 == cols: rejected; == cols - 1: accepted
    for tag, ur, gate in (("endu_eq", w - 11, "endu>=cols"), ("endu_below", w - 12, "accepted")):
        il, ir = F.pair(ur + 5.0, y, float(ur), sad=9, tag=tag)
        F.expect(tag, best_idx=ir, gate="accepted" if gate == "accepted" else gate)
        y += 16
    # the same at octave 2 (the pixels there are the pyramid's: only the gate is asserted)
    lw = F.sizes[2][0]
    for tag, tgt in (("endu2_eq", lw - 11), ("endu2_below", lw - 12)):
        d = F.rand_desc()
        ir = F.add_right(_x_for_scaled(F, 2, tgt), y, 2, d)
        F.add_left(_x_for_scaled(F, 2, tgt + 4), y, 2, d, tag)
        F.expect(tag, best_idx=ir, gate="endu>=cols" if tgt == lw - 11 else (lambda g: g != "endu>=cols"),
                 sads=(lambda s: s is None) if tgt == lw - 11 else (lambda s: s is not None))
        y += 16
    # bestincR -5, -4, +4, +5
    for i, (e, gate) in enumerate(((-5, "bestincR=-L"), (-4, "accepted"), (4, "accepted"), (5, "bestincR=+L"))):
        tag = "inc%+d" % e
        F.pair(60.0 + 40 * i, y, 50.0 + 40 * i, e=e, sad=7, tag=tag)
        F.expect(tag, best_inc=e, gate="accepted" if gate == "accepted" else gate)
    y += 16
    # SAD 0 at increments 1 and 2: the first wins, dist2 == dist3, deltaR = +0.5
    F.pair(60.0, y, 50.0, e=1, kind="two_minima", tag="two_minima")
    F.expect("two_minima", best_inc=1, delta_r=0.5, sads=lambda s: s[6] == 0 and s[7] == 0 and s[5] > 0)
    # a flat patch: every SAD 0, rejected at -L
    F.pair(130.0, y, 120.0, kind="flat", tag="flat")
    F.expect("flat", sads=[0] * 11, gate="bestincR=-L")
    y += 16
    # 0 / 255: a checkerboard against its opposite phase, and the largest sum there is (120 * 510)
    F.pair(60.0, y, 50.0, kind="checker", tag="checker")
    F.expect("checker", sads=lambda s: max(s) == 60 * 510)
    F.pair(130.0, y, 120.0, kind="extreme", tag="extreme")
    F.expect("extreme", sads=lambda s: max(s) == 120 * 510 and s[5] == 120 * 510)
    y += 16
    # deltaR == 0 with a disparity inside the range
    F.pair(70.0, y, 60.0, kind="symmetric", tag="delta0")
    F.expect("delta0", delta_r=0, gate="accepted", zero_branch=False)
    # a mirror-symmetric patch, zero shift, integer uL: disparity exactly 0, the 0.01 branch
    F.pair(140.0, y, 140.0, kind="symmetric", tag="zero")
    F.expect("zero", delta_r=0, zero_branch=True, gate="accepted")
    y += 16
    # deltaR next to its other end: dist1 = 1, dist2 = 0, dist3 large
    F.pair(70.0, y, 60.0, kind="near_minus", tag="delta_neg")
    F.ballast(6, y + 16)
    F.expect("delta_neg", best_inc=0, sads=lambda s: s[4] == 1 and s[5] == 0 and s[6] > 100, delta_r=lambda v: -0.5 < v < -0.49)
    return F.finish()


def frame_median(w, h, name, sads, seed, **want):
    """accepted matches with exactly these best SADs, in this order"""
    F = Frame(name, w, h, seed)
    for i, s in enumerate(sads):
        x, y = 40.0 + 40 * (i % 4), 12.0 + 16 * (i // 4)
        F.pair(x, y, x - 9.0, sad=s, tag="m%d" % i)
        F.expect("m%d" % i, sad=s)
    if not sads:  # nothing is accepted: one key rejected at +L keeps the frame from being empty
        F.pair(60.0, 12.0, 50.0, e=5, tag="none")
        F.expect("none", gate="bestincR=+L")
    F.add_left(200.0, 200.0, 0, None, "frame")
    F.expect("frame", frame=lambda c: all((c.median, c.n_accepted, c.count("median"))[i] == v
                                          for i, v in enumerate((want.get("median"), len(sads), want.get("rejected"))) if v is not None))
    return F.finish()


def median_frames(w, h):
    th21 = [10, 10, 10, 10, 20, 21, 22]  # median 10, thDist = 1.5f * 1.4f * 10: the oracle decides the side of 21
    th42 = [20, 20, 20, 20, 41, 42, 43]
    return [
        frame_median(w, h, "median_n0", [], 10),
        frame_median(w, h, "median_n1", [10], 11, median=10.0, rejected=0),
        frame_median(w, h, "median_n2", [10, 30], 12, median=30.0, rejected=0),       # (n - 1) / 2 would give 10 and reject 30
        frame_median(w, h, "median_n3", [30, 10, 20], 13, median=20.0, rejected=0),
        frame_median(w, h, "median_n4", [40, 10, 30, 12], 14, median=30.0, rejected=0),  # (n - 1) / 2: 12, rejects 30 and 40
        frame_median(w, h, "median_equal", [15] * 6, 15, median=15.0, rejected=0),
        frame_median(w, h, "median_zero", [0] * 6, 16, median=0.0, rejected=6),        # thDist = 0: nothing is below it
        frame_median(w, h, "median_set6", [10, 20, 10, 22, 10, 21], 17, median=20.0, rejected=0),
        frame_median(w, h, "median_th21", th21[::-1], 18, median=10.0),
        frame_median(w, h, "median_th42", th42, 19, median=20.0),
    ]


def frame_big(w, h):
    """more than 2048 left keys (the registers of k_stereo_median hold 2048): 1100 keys of SAD 10 and 948 of SAD 25 fill
    the first 2048 places, 400 of SAD 30 follow.  The median of all is 25 (thDist 52.5: nothing is rejected); over the
    first 2048 it is 10 (thDist 21: the 25s and 30s would go)."""
    F = Frame("big", w, h, 20)
    slots = []
    for i, s in enumerate((10, 25, 30)):
        x, y = 60.0 + 50 * i, 40.0
        d = F.rand_desc()
        F.paint(x, x - 9.0, y, sad=s)
        F.add_right(x - 9.0, y, 0, d)
        slots.append((x, y, d, s))
    order = [0] * 1100 + [1] * 948 + [2] * 400
    for j, s in enumerate(order):
        x, y, d, _ = slots[s]
        F.add_left(x, y, 0, F.flip(d, j % 8, 8 * (j % 31)), "big0" if j == 0 else None)

    def whole(c):
        first = sorted(r["sad"] for r in c[:2048] if r["sad"] is not None)
        m2048 = first[len(first) // 2]
        th2048 = stereo_ref.f32(stereo_ref.f32(stereo_ref.f32(1.5) * stereo_ref.f32(1.4)) * stereo_ref.f32(m2048))
        rejected_2048 = {i for i, r in enumerate(c) if r["sad"] is not None and not stereo_ref.f32(r["sad"]) < th2048}
        rejected = {i for i, r in enumerate(c) if r["gate"] == "median"}
        return len(c) == 2448 and c.n_accepted == 2448 and c.median == 25.0 and m2048 == 10 and rejected != rejected_2048
    F.expect("big0", frame=whole)
    return F.finish()


def frame_big_reject(w, h):
    """the other way round: the median of the first 2048 would keep what the true median rejects"""
    F = Frame("big_reject", w, h, 21)
    slots = []
    for i, s in enumerate((40, 30, 10)):
        x, y = 60.0 + 50 * i, 40.0
        d = F.rand_desc()
        F.paint(x, x - 9.0, y, sad=s)
        F.add_right(x - 9.0, y, 0, d)
        slots.append((x, y, d, s))
    order = [0] * 100 + [1] * 1948 + [2] * 2100  # first 2048: median 30 (thDist 63); all: median 10 (thDist 21)
    for j, s in enumerate(order):
        x, y, d, _ = slots[s]
        F.add_left(x, y, 0, F.flip(d, j % 8, 8 * (j % 31)), "big0" if j == 0 else None)
    F.expect("big0", frame=lambda c: c.median == 10.0 and c.count("median") == 2048 and c.n_accepted == 4148)
    return F.finish()


def frame_empty_left(w, h):
    F = Frame("empty_left", w, h, 30)
    F.add_right(100, 50.0)
    return F.finish()


def frame_no_right(w, h):
    F = Frame("no_right", w, h, 31)
    for i in range(5):
        F.add_left(40.0 + 30 * i, 60.0, 0, None, "k%d" % i)
        F.expect("k%d" % i, gate="no_candidate")
    return F.finish()


def frame_tall(w, h):
    """rows beyond 1024 (the prefix sum of the 1024-thread row kernel takes more than one row a thread)"""
    F = Frame("tall", w, h, 40)
    for i, y in enumerate((h - 7.0, h - 6.0, 1000.4, 512.0, 20.0)):  # h - 6: the last row a patch of octave 0 fits in
        x = 100.0 + 60 * i
        F.pair(x, y, x - 9.0 - i, sad=5 + i, tag="row%d" % int(y))
        F.expect("row%d" % int(y), row=int(y), n_gated=1, gate="accepted", sad=5 + i)
    d = F.rand_desc()  # the last row of all: only a key with x < 0 is in the domain there
    F.add_right(50, h - 1.0, 0, d)
    F.add_left(-3.0, h - 1.0, 0, d, "last_row")
    F.expect("last_row", row=h - 1, n_cand=1, gate="maxU<0")
    F.add_left(300.0, 1010.0, 0, None, "gap")
    F.expect("gap", gate="no_candidate")
    _stack(F, 960.0, 33, 32, "tall33", ul=500.0)
    return F.finish()


def all_frames(w, h):
    """every planted frame of one image size, the special ones first (a batch of 16 holds them all)"""
    return [frame_empty_left(w, h), frame_no_right(w, h), frame_big(w, h), frame_counts(w, h), frame_big_reject(w, h),
            frame_rows(w, h), frame_counts_first(w, h), frame_ties(w, h), frame_tie_order(w, h), frame_gates(w, h), frame_refine(w, h), frame_oct7(w, h)] + median_frames(w, h)
