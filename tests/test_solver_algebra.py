"""The lane functions of the relocalisation and loop-verification solvers (pnp_device.h, sim3_solver_device.h), called
directly and compared with a 50-digit reference (tests/solver_ref.py) on named cases (tests/solver_cases.py).
tests/hip_unit/solver_algebra_test.hip evaluates on the device, tests/emul/{pnp,sim3}_emul.cc on the host; nothing is
compared in C++.

Three statements meet here: the 50-digit reference (written from the reference's text: branches and float roundings as
written, the linear algebra from its definitions), the LAPACK / numpy restatements (tests/reloc_ref.py,
tests/loop_ref.py, numpy.linalg for the helpers), whose error against the 50-digit value is E_lapack(case), and the
code under test.  The device -- and the host build of the same headers, which is how the cases are debugged without a
GPU -- stays within 4 x max(E_lapack(case), dim x 2^-52) of the reference output's max-norm, dim the dimension of the
matrix at work (2 for pnp_rot, 3, 4, 6 for the least squares, 12 for compute_pose).  Values the reference holds as
float and inlier decisions are equal, unless a value rounded out of double arithmetic lies within 1e-12 of a rounding
boundary (at most 2 per 1000).  Where an eigenvector is not unique the invariants are compared by the same rule.
pnp_epnp runs in its real shape (16 lanes a workgroup, the two LDS work arrays, a partly filled last workgroup) and
hands out the values that decide its branches through PNP_TAP, a macro that is empty in the library.  Whole-EPnP parity
is asked for n >= 6 (What EPnP leaves open); the n = 4, 5 cases are checked for properties and lanes.

Found by these tests and fixed in pnp_device.h:
  * pnp_lstsq6 skipped the reflection of a zero column but went on to the next row, so the unknowns behind it were no
    minimiser (zero-column-0 of pnp_lstsq6<3>: x off by 2.3 of its max-norm, ratio to the bound 1.7e14).  An
    axis-aligned planar scene has two such columns in the first initial guess; with rank-deficient systems the
    reference's cv::solve(DECOMP_SVD) returns the minimiser of smallest norm, the device returned another one
    (proportional-columns of <4>: residual 0.23 |b| above the smallest).  Now negligible columns move behind the
    others and the smallest-norm minimiser is returned; full-rank systems take the old path, bit for bit.
  * pnp_polar3 took +1 for the third column's sign where that column vanishes (B of rank 2 to the last bit: map points
    with one coordinate constant), which can make R a reflection that compute_pose's row flip turns into a wrong
    pose: planar-axis-aligned came out 1.70 m / 0.43 rad from the truth (the restatement: 1.1e-6 m).  The sign is now
    the one that makes R a rotation.
  * rho was computed from control points to which the centroid had been added, the barycentric coordinates from the
    unrounded ones: at a world offset of 1e4 m the pose was 1e-13 off, 86 times the restatement's error in the median
    of 8 scenes (ratio to the bound up to 70).  The control points are now kept relative to the centroid: 0.7 times.
  The existing PnP tests pass as before.

Deliberate faults, each tried on a scratch copy and not kept.  `sn` negated in pnp_rot: pnp_rot (67 of 70 cases; the
rest have sn = 0 or compare cs only), pnp_eig3 d / U / invariants, pnp_polar3 (35), pnp_epnp (22), the eig3 and epnp
branch assertions, test_relocalization's host test; nothing of lstsq, alphas, project, check_inliers, lanes, s3s_*.
`64 * w` dropped from pnp_check_inliers' index: pnp_check_inliers n = 65, 127, 128, 129 (both fills: 8 cases, 172
bits) and nothing else; through the C ABI on the device, test_pnp_tables_across_mask_words and
test_pnp_refine_parity_across_mask_words only.  `row * C.words` -> `row` in k_pnp_hypotheses, on the device:
test_pnp_tables_across_mask_words (n = 65 first), test_pnp_batch_independence_across_mask_words and the two chain
tests whose candidates have more than 64 matches; every one-word test passes.

Branches without a case: `vv == 0` in pnp_lstsq6 cannot be entered -- alpha takes the sign opposite to A[k][k], so
|A[k][k] - alpha| >= the column's length, which is positive there; the cases column-reduced-to-its-pivot-* and
upper-triangular run the reflection of a column that is its pivot alone.  x[1] < 0 and z0 < 0 carry the signs of the
eigenvectors, which are the eigen-solver's own, so they are asserted from the evaluator's taps and not from the
reference.  x[0] < 0 needed 5 px of noise on 6 points (solver_cases.BRANCH_SEEDS).

Measured on an MI355X (E_lapack worst, at which case; median; the device's worst ratio to its bound; the host build's
ratios are the same at the printed digits):

  pnp_lstsq6<3>          4.2e-15 pivot-zero                   4.5e-16   0.428
  pnp_lstsq6<4>          3.4e-15 generic-8                    6.9e-16   0.291
  pnp_lstsq6<5>          5.1e-14 upper-triangular             8.0e-16   0.648
  pnp_rot                2.0e-16 generic-58                   5.6e-17   0.113
  pnp_eig3 d             7.5e-16 scatter-5                    1.3e-16   0.085
  pnp_eig3 U             8.8e-13 generic-2 column 0           3.6e-16   0.365
  pnp_eig3 invariants    1.3e-15 rank-1 residual              2.5e-16   0.435
  pnp_polar3             8.3e-16 generic-5                    4.3e-16   0.257
  pnp_polar3 R^T R = I   1.5e-15 generic-5                    7.6e-16   0.364
  pnp_alphas             3.3e-16 planar-frame                 9.7e-17   0.125
  pnp_project            3.5e-16 generic-29                   5.2e-17   0.130   0 of 38 excused
  pnp_check_inliers      0 of 1544 decisions excused; guard words untouched, words holding ones overwritten
  pnp_epnp (n >= 6)      5.7e-10 planar-tilted                2.1e-14   0.639 (generic-n=60)
  pnp_epnp lanes         every case the same bytes in lanes 0, 7, 15, among other neighbours, in the last workgroup
  s3s_top_eigenvector    1.1e-14 horn/generic-8               2.4e-16   0.308
    invariants           8.1e-16 horn/generic-9 residual      2.5e-18   0.166
  s3s_horn               2.2e-14 generic-8 R                  2.5e-16   0.655 (generic-17 t)
    invariants           3.3e-16 collinear-...-fixed-scale    1.5e-16   0.188
  s3s_pose               2.9e-16 generic-12                   1.1e-16   0.108
  s3s_project            0 of 144 float values excused (pinhole, Radtan, KB8, a pinhole behind a body transform)
  s3s_dist2              0 of 42 excused
  s3s_is_inlier          0 of 49 decisions excused
  C ABI across mask words (tests/test_relocalization.py): pass B on 6 ... 130 of 130 correspondences against the
  restated EPnP 4.1e-14 m, 7.5e-15 rad

The 50-digit statements against exact definitions (test_reference_against_exact_definitions): Horn on noise-free
triples gives the generating similarity within 1e-12; compute_pose on the noise-free scenes gives the generating pose
within 1e-4 (the float rounding of map points and pixels).
"""
import atexit
import ctypes
import functools
import os
import shutil
import subprocess
import tempfile

import mpmath
import numpy as np
import pytest
from mpmath import mpf

from tests import algebra_cases as AC
from tests import loop_ref
from tests import reloc_ref
from tests import solver_cases as SC
from tests import solver_ref as SR
from tests.test_device_algebra import EPS, EXCUSE_CAP, EXCUSE_MARGIN, cam_tables, hipcc_flags, read_blob, rel_err, write_blob

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
f32 = np.float32
NCS = (3, 4, 5)
TAP_SLOTS = 48
GUARD = 0x5A5A5A5A5A5A5A5A


def bound(e_lapack, dim):
    """the device's (and the host build's) allowance: 4 x max(E_lapack(case), dim x 2^-52)"""
    return 4 * max(e_lapack, dim * EPS)


def V(x):
    return [mpf(float(t)) for t in np.asarray(x, np.float64).reshape(-1)]


def mat(x):
    x = np.asarray(x, np.float64)
    return SR.M(x.reshape(-1), x.shape[0], x.shape[1])


# ------------------------------------------------------------------ the program, its inputs, the two evaluators
@functools.lru_cache(maxsize=None)
def built_program():
    flags, hipcc = hipcc_flags()
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc") or hipcc
    d = tempfile.mkdtemp(prefix="solver_algebra_")
    atexit.register(shutil.rmtree, d, True)
    exe = os.path.join(d, "solver_algebra_test")
    r = subprocess.run([hipcc] + flags + ["-o", exe, os.path.join(HERE, "hip_unit", "solver_algebra_test.hip")],
                       capture_output=True, text=True)
    if r.returncode != 0:
        return None, r.stdout + r.stderr
    return exe, r.stdout + r.stderr


@functools.lru_cache(maxsize=None)
def epnp_case_list():
    return SC.epnp_cases() + SC.epnp_small_cases()


@functools.lru_cache(maxsize=None)
def inlier_cases():
    """s3s_is_inlier: each pair of solver_cases.inlier_pairs at its own thresholds -- generous, err1 met exactly and
    missed by an ulp, err2 the same -- and at a pose that is not finite.  (name, c1, c2, T24, X1, X2, me1, me2)"""
    _, cams, _ = AC.cameras()
    out = []
    for name, c1, c2, R, t, s, X1, X2 in SC.inlier_pairs():
        T = SR.sim3_pose([V(r) for r in R], V(t), mpf(s))
        T24 = np.array([float(x) for x in T])
        Tm = [mpf(x) for x in T24]
        A12, t12 = [Tm[3 * r:3 * r + 3] for r in range(3)], Tm[9:12]
        A21, t21 = [Tm[12 + 3 * r:15 + 3 * r] for r in range(3)], Tm[21:24]
        e1 = SR.dist2(SR.sim3_project(cams[c1], None, None, V(X1))[0], SR.sim3_project(cams[c1], A12, t12, V(X2))[0])[0]
        e2 = SR.dist2(SR.sim3_project(cams[c2], A21, t21, V(X1))[0], SR.sim3_project(cams[c2], None, None, V(X2))[0])[0]
        e1, e2 = float(e1), float(e2)
        up = lambda x: float(np.nextafter(f32(x), f32(np.inf)))
        big = 1e6
        for tag, me1, me2 in (("generous", big, big), ("err1-equals-threshold", e1, big), ("err1-one-ulp-below", up(e1), big),
                              ("err2-equals-threshold", big, e2), ("err2-one-ulp-below", big, up(e2)), ("tight", 0.5 * e1, big)):
            out.append((name + "/" + tag, c1, c2, T24, X1, X2, me1, me2))
    name, c1, c2, R, t, s, X1, X2 = SC.inlier_pairs()[0]
    out.append(("pose-not-finite", c1, c2, np.concatenate([np.eye(3).reshape(-1), [np.nan] * 3, np.full(12, np.nan)]), X1, X2,
                1e30, 1e30))
    return out


@functools.lru_cache(maxsize=None)
def program_inputs():
    inp = {}
    for nc in NCS:
        cs = SC.lstsq_cases(nc)
        inp["L.A%d" % nc] = np.array([c[1] for c in cs], np.float64)
        inp["L.b%d" % nc] = np.array([c[2] for c in cs], np.float64)
    inp["R.abg"] = np.array([c[1:4] for c in SC.rot_cases()], np.float64)
    inp["E.S"] = np.array([c[1] for c in SC.eig3_cases()], np.float64)
    inp["P.B"] = np.array([c[1] for c in SC.polar3_cases()], np.float64)
    al = SC.alphas_cases()
    inp["Q.frame"] = np.array([np.concatenate([c[1], np.asarray(c[2]).reshape(-1)]) for c in al], np.float64)
    inp["Q.X"] = np.array([c[3] for c in al], np.float64)
    pj = SC.project_cases()
    inp["J.K"] = np.array([c[1] for c in pj], np.float64)
    inp["J.Rt"] = np.array([np.concatenate([np.asarray(c[2]).reshape(-1), c[3]]) for c in pj], np.float64)
    inp["J.X"] = np.array([c[4] for c in pj], np.float64)
    ck = SC.check_cases()
    off, case = 0, []
    for c in ck:
        case.append((off, len(c[4]), c[7]))
        off += len(c[4])
    inp["I.case"] = np.array(case, np.int32)
    inp["I.K"] = np.array([c[1] for c in ck], np.float64)
    inp["I.Rt"] = np.array([np.concatenate([np.asarray(c[2], np.float64).reshape(-1), c[3]]) for c in ck], np.float64)
    inp["I.Xw"] = np.concatenate([c[4] for c in ck]).astype(np.float64)
    inp["I.uv"] = np.concatenate([c[5] for c in ck]).astype(np.float64)
    inp["I.max_err"] = np.concatenate([c[6] for c in ck]).astype(np.float64)
    ep = epnp_case_list()
    cand, idx_off, off, ioff = [], [], 0, 0
    for c in ep:
        cand.append((off, len(c[2])))
        idx_off.append(ioff)
        off, ioff = off + len(c[2]), ioff + len(c[4])
    jobs = SC.epnp_jobs([c[0] for c in ep])
    inp["X.job"] = np.array([(j, idx_off[j], len(ep[j][4])) for j in jobs], np.int32)
    inp["X.cand"] = np.array(cand, np.int32)
    inp["X.cand_K"] = np.array([c[1] for c in ep], np.float64)
    inp["X.Xw"] = np.concatenate([c[2] for c in ep]).astype(np.float64)
    inp["X.uv"] = np.concatenate([c[3] for c in ep]).astype(np.float64)
    inp["X.idx"] = np.concatenate([c[4] for c in ep]).astype(np.int32)
    inp["T.N"] = np.array([c[1] for c in SC.top_cases()], np.float64)
    hc = SC.horn_cases()
    inp["H.P1"] = np.array([c[1] for c in hc], np.float64)
    inp["H.P2"] = np.array([c[2] for c in hc], np.float64)
    inp["H.fix_scale"] = np.array([int(c[3]) for c in hc], np.int32)
    inp["S.Rts"] = np.array([np.concatenate([c[1].reshape(-1), c[2], [c[3]]]) for c in SC.pose_cases()], np.float64)
    inp["C.cam_f64"], inp["C.cam_i32"] = cam_tables()
    vc = SC.sim3_project_cases()
    inp["V.cam"] = np.array([(c[1], int(c[2] is not None)) for c in vc], np.int32)
    inp["V.A"] = np.array([np.concatenate([np.asarray(c[2]).reshape(-1), c[3]]) if c[2] is not None else np.zeros(12) for c in vc])
    inp["V.X"] = np.array([c[4] for c in vc], np.float64)
    dc = SC.dist2_cases()
    inp["D.ab"] = np.array([np.concatenate([c[1], c[2]]) for c in dc], np.float64)
    ic = inlier_cases()
    inp["N.cam"] = np.array([(c[1], c[2]) for c in ic], np.int32)
    inp["N.T"] = np.array([c[3] for c in ic], np.float64)
    inp["N.X"] = np.array([np.concatenate([c[4], c[5]]) for c in ic], np.float64)
    inp["N.max_err"] = np.array([(f32(c[6]), f32(c[7])) for c in ic], np.float64)
    return inp


@functools.lru_cache(maxsize=None)
def device_run():
    """("ok", outputs) or ("failed", message): built once, fed once, run once; a failure is cached and every test
    reports it without starting the program again"""
    exe, log = built_program()
    if exe is None:
        return "failed", "hipcc failed:\n" + log
    d = os.path.dirname(exe)
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    write_blob(fin, program_inputs())
    try:
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired as e:
        return "failed", "timed out: %s" % e
    if r.returncode != 0:
        return "failed", "exit code %d\n%s%s" % (r.returncode, r.stdout, r.stderr)
    return "ok", read_blob(fout)


def device_outputs():
    st, out = device_run()
    assert st == "ok", out
    return out


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


@functools.lru_cache(maxsize=None)
def _emul_libs():
    libs = []
    csrc = os.path.join(ROOT, "vieo_slam_amd", "csrc")
    for stem, hdrs in (("pnp", ["pnp_device.h"]), ("sim3", ["sim3_solver_device.h", "cam_project.h"])):
        out = os.path.join(HERE, "emul", "lib%s_emul.so" % stem)
        deps = [os.path.join(HERE, "emul", "%s_emul.cc" % stem)] + [os.path.join(csrc, h) for h in hdrs]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", out, deps[0], "-lm"])
        libs.append(ctypes.CDLL(out))
    libs[1].emul_s3s_dist2.restype = ctypes.c_float
    return libs


def host_epnp(K, Xw, uv, idx, lane=0, fill=0.0):
    """pnp_epnp of the host build in a lane of its work area: (Rt[12], tap[48])"""
    P, _ = _emul_libs()
    Xw, uv, K = np.ascontiguousarray(Xw, f32), np.ascontiguousarray(uv, f32), np.ascontiguousarray(K, f32)
    idx = np.ascontiguousarray(idx, np.int32)
    Rt, tap = np.zeros(12), np.zeros(TAP_SLOTS)
    P.emul_pnp_epnp_lane(_p(Xw), _p(uv), len(Xw), _p(K), _p(idx), len(idx), int(lane), ctypes.c_double(fill), _p(Rt), _p(tap))
    return Rt, tap


@functools.lru_cache(maxsize=None)
def host_outputs():
    """the arrays the program writes, from the host build of the same headers"""
    P, S = _emul_libs()
    inp = program_inputs()
    out = {}
    for nc in NCS:
        A, b = inp["L.A%d" % nc], inp["L.b%d" % nc]
        x = np.zeros((len(A), nc))
        for k in range(len(A)):
            assert P.emul_pnp_lstsq6(nc, _p(A[k]), _p(b[k]), _p(x[k])) == 0
        out["L.pnp_lstsq6<%d>" % nc] = x.reshape(-1)

    def each(fn, n, width, *arrays, dtype=np.float64):
        o = np.zeros((n, width), dtype)
        for k in range(n):
            fn(*[_p(a[k]) for a in arrays], _p(o[k]))
        return o.astype(np.float64).reshape(-1)

    out["R.pnp_rot"] = each(P.emul_pnp_rot, len(inp["R.abg"]), 3, inp["R.abg"])
    S_, d, U = inp["E.S"], np.zeros((len(inp["E.S"]), 3)), np.zeros((len(inp["E.S"]), 9))
    for k in range(len(S_)):
        P.emul_pnp_eig3(_p(S_[k]), _p(d[k]), _p(U[k]))
    out["E.pnp_eig3.d"], out["E.pnp_eig3.U"] = d.reshape(-1), U.reshape(-1)
    out["P.pnp_polar3"] = each(P.emul_pnp_polar3, len(inp["P.B"]), 9, inp["P.B"])
    out["Q.pnp_alphas"] = each(P.emul_pnp_alphas, len(inp["Q.frame"]), 4, inp["Q.frame"], inp["Q.X"].astype(f32))
    out["J.pnp_project"] = each(P.emul_pnp_project, len(inp["J.K"]), 2, inp["J.K"].astype(f32), inp["J.Rt"], inp["J.X"].astype(f32))
    Xw, uv, me = inp["I.Xw"].astype(f32), inp["I.uv"].astype(f32), inp["I.max_err"].astype(f32)
    P.emul_pnp_check.restype = ctypes.c_int
    cnt, halves = [], []
    for k, (off, n, fill) in enumerate(inp["I.case"]):
        words = np.full(4, GUARD, np.uint64)
        words[:(n + 63) // 64] = 0xFFFFFFFFFFFFFFFF if fill else 0
        Kf = inp["I.K"][k].astype(f32)
        a, b, c = (np.ascontiguousarray(x[off:off + n]) for x in (Xw, uv, me))
        cnt.append(P.emul_pnp_check(_p(a), _p(b), _p(c), int(n), _p(Kf), _p(inp["I.Rt"][k]), _p(words)))
        halves.append(words.view(np.uint32).astype(np.float64))
    out["I.count"], out["I.mask_halves"] = np.array(cnt, np.float64), np.concatenate(halves)
    ep = epnp_case_list()
    Rt, tap = [], []
    for lane, (j, _, _) in enumerate(inp["X.job"]):
        r, t = host_epnp(ep[j][1], ep[j][2], ep[j][3], ep[j][4], lane % 16, float(lane))
        Rt.append(r), tap.append(t)
    pad = (-len(tap)) % 16
    out["X.Rt"], out["X.tap"] = np.concatenate(Rt), np.concatenate(tap + [np.zeros(TAP_SLOTS)] * pad)
    out["T.s3s_top_eigenvector"] = each(S.emul_s3s_top_eigenvector, len(inp["T.N"]), 4, inp["T.N"])
    h = np.zeros((len(inp["H.P1"]), 13))
    for k in range(len(h)):
        S.emul_s3s_horn(_p(inp["H.P1"][k]), _p(inp["H.P2"][k]), int(inp["H.fix_scale"][k]), _p(h[k]))
    out["H.s3s_horn"] = h.reshape(-1)
    out["S.s3s_pose"] = each(S.emul_s3s_pose, len(inp["S.Rts"]), 24, inp["S.Rts"])
    cf, ci = inp["C.cam_f64"], inp["C.cam_i32"]
    uvs = np.zeros((len(inp["V.cam"]), 2), f32)
    VX = inp["V.X"].astype(f32)
    for k, (c, has) in enumerate(inp["V.cam"]):
        S.emul_s3s_project(_p(cf[c]), _p(ci[c]), int(has), _p(inp["V.A"][k]), _p(VX[k]), _p(uvs[k]))
    out["V.s3s_project"] = uvs.astype(np.float64).reshape(-1)
    ab = inp["D.ab"].astype(f32)
    out["D.s3s_dist2"] = np.array([S.emul_s3s_dist2(_p(ab[k])) for k in range(len(ab))], np.float64)
    NX, Nme = inp["N.X"].astype(f32), inp["N.max_err"].astype(f32)
    out["N.s3s_is_inlier"] = np.array([S.emul_s3s_is_inlier(_p(inp["N.T"][k]), _p(cf[c1]), _p(ci[c1]), _p(cf[c2]), _p(ci[c2]),
                                                            _p(NX[k]), _p(Nme[k])) for k, (c1, c2) in enumerate(inp["N.cam"])],
                                      np.float64)
    return out


# ------------------------------------------------------------------ reports
class Report:
    """what one family's comparison found: rows (case, error, E_lapack, bound), float / decision mismatches with their
    margins; the checks every evaluator has to pass"""

    def __init__(self, family, dim):
        self.family, self.dim, self.rows, self.values, self.excused, self.bad = family, dim, [], 0, [], []

    def add(self, case, err, e_lapack, what=""):
        b = bound(e_lapack, self.dim)
        self.rows.append((case + what, err, e_lapack, b))
        if not err <= b:
            self.bad.append("%s/%s%s: error %.3g, bound %.3g (E_lapack %.3g)" % (self.family, case, what, err, b, e_lapack))

    def exact(self, case, got, want, margin):
        """a float value or a decision that has to equal the reference's unless that is within EXCUSE_MARGIN of a
        rounding boundary or threshold"""
        self.values += 1
        if got == want:
            return
        if margin < EXCUSE_MARGIN:
            self.excused.append(case)
        else:
            self.bad.append("%s/%s: %r, the reference has %r (margin %.3g)" % (self.family, case, got, want, float(margin)))

    def require(self, ok, case, what):
        if not ok:
            self.bad.append("%s/%s: %s" % (self.family, case, what))

    def line(self, who):
        s = "%-22s" % self.family
        if self.rows:
            e = np.array([r[2] for r in self.rows])
            k = int(e.argmax())
            ratios = [r[1] / r[3] for r in self.rows]
            s += " E_lapack worst %.2g (%s), median %.2g; %s worst ratio %.3f (%s)" % (
                e.max(), self.rows[k][0], float(np.median(e)), who, max(ratios), self.rows[int(np.argmax(ratios))][0])
        if self.values:
            s += " %d of %d values excused" % (len(self.excused), self.values)
        return s


def finish(reports, who):
    bad = []
    for r in reports:
        print(r.line(who))
        bad += r.bad
        if r.values and len(r.excused) > max(EXCUSE_CAP * r.values, 0):
            bad.append("%s: %d of %d values excused: %s" % (r.family, len(r.excused), r.values, r.excused[:5]))
    per_family = {}
    for b in bad:
        per_family.setdefault(b.split("/")[0].split(":")[0], set()).add(b.split(":")[0].split("[")[0])
    summary = "%d failures: %s" % (len(bad), ", ".join("%s (%d cases)" % (k, len(v)) for k, v in sorted(per_family.items())))
    assert not bad, summary + "\n" + "\n".join(bad[:40])


def _align(x, ref):
    """x with the sign that brings it closest to ref (a direction whose sign is not defined)"""
    x = np.asarray(x, np.float64)
    r = np.array([float(t) for t in ref])
    return -x if np.dot(x, r) < 0 else x


# ------------------------------------------------------------------ L. pnp_lstsq6
@functools.lru_cache(maxsize=None)
def ref_lstsq():
    """per nc and case: ("x", reference x, E_lapack) or ("residual", A, b, smallest residual, |b|, E_lapack)"""
    out = {}
    for nc in NCS:
        rows = []
        for name, A, b, kind in SC.lstsq_cases(nc):
            lap = np.linalg.lstsq(A, b, rcond=None)[0]
            Am, bm = mat(A), mpmath.matrix(V(b))
            if kind == "deficient":
                keep = list(range(nc - 1))
                res = SR.lstsq(mat(A[:, keep]), bm)[1]
                nb = mpmath.norm(bm, 2)
                rows.append(("residual", Am, bm, res, nb, float((SR.residual(Am, bm, lap) - res) / nb)))
                continue
            if kind == "full":
                x = SR.lstsq(Am, bm)[0]
            else:
                keep = [c for c in range(nc) if c != kind[1]]
                x = SR.lstsq(mat(A[:, keep]), bm)[0]
                x.insert(kind[1], mpf(0))
                lap = np.linalg.lstsq(A[:, keep], b, rcond=None)[0]
                lap = np.insert(lap, kind[1], 0.0)
            rows.append(("x", x, rel_err(lap, x)))
        out[nc] = rows
    return out


def check_lstsq(out):
    reports = []
    for nc in NCS:
        rep = Report("pnp_lstsq6<%d>" % nc, 6)
        x = out["L.pnp_lstsq6<%d>" % nc].reshape(-1, nc)
        for k, (case, row) in enumerate(zip(SC.lstsq_cases(nc), ref_lstsq()[nc])):
            if row[0] == "x":
                rep.add(case[0], rel_err(x[k], row[1]), row[2])
                if isinstance(case[3], tuple):
                    rep.require(x[k][case[3][1]] == 0.0, case[0], "x of the zero column is %r" % x[k][case[3][1]])
            else:
                _, Am, bm, res, nb, e_lap = row
                rep.require(np.isfinite(x[k]).all(), case[0], "x is not finite")
                if np.isfinite(x[k]).all():
                    rep.add(case[0], float((SR.residual(Am, bm, x[k]) - res) / nb), e_lap, " (residual above the smallest)")
        reports.append(rep)
    return reports


# ------------------------------------------------------------------ R. pnp_rot
def _rot_restated(a, b, g):
    """the same root in Python floats, through hypot (no overflow)"""
    import math
    zeta = (b - a) / (2 * g)
    t = math.copysign(1.0, zeta) / (abs(zeta) + math.hypot(1.0, zeta)) if zeta != 0 else 1.0
    cs = 1 / math.hypot(1.0, t)
    return [t, cs, cs * t]


@functools.lru_cache(maxsize=None)
def ref_rot():
    return [(SR.jacobi_rot(mpf(a), mpf(b), mpf(g)), None) for _, a, b, g in SC.rot_cases()]


def check_rot(out):
    # a 2 x 2 problem: dim = 2.  t takes 5 roundings, cs 4 more, sn one more; 8 x 2^-52 covers the chain
    rep = Report("pnp_rot", 2)
    got = out["R.pnp_rot"].reshape(-1, 3)
    for k, ((name, a, b, g), (ref, _)) in enumerate(zip(SC.rot_cases(), ref_rot())):
        rep.add(name, rel_err(got[k], ref), rel_err(_rot_restated(a, b, g), ref))
        t, cs, sn = got[k]
        rep.require(cs > 0 and abs(t) <= 1 and (t == 0 or (t > 0) == ((b - a) / g >= 0)), name, "t = %r, cs = %r" % (t, cs))
        # the rotation annihilates g: (cs^2 - sn^2) g + cs sn (a - b) = 0
        resid = abs((mpf(cs) ** 2 - mpf(sn) ** 2) * mpf(g) + mpf(cs) * mpf(sn) * (mpf(a) - mpf(b)))
        rep.require(resid <= 8 * EPS * max(abs(a), abs(b), abs(g)), name, "leaves %.3g of the off-diagonal" % float(resid))
    return [rep]


# ------------------------------------------------------------------ E. pnp_eig3
def _eig_invariants(S, d, U):
    """(|S u - d u| over |S|, |U^T U - I|) for doubles d, U against the 50-digit S"""
    Um = mat(np.asarray(U).reshape(3, 3))
    D = mpmath.diag([mpf(float(t)) for t in d])
    nS = max(mpmath.norm(S, "inf"), mpf(10) ** -300)
    return float(mpmath.norm(S * Um - Um * D, "inf") / nS), float(mpmath.norm(Um.T * Um - mpmath.eye(3), "inf"))


@functools.lru_cache(maxsize=None)
def ref_eig3():
    rows = []
    for name, S, kind in SC.eig3_cases():
        Sm = mat(S)
        w, U = SR.eig_desc(Sm)
        lw, lU = np.linalg.eigh(S)
        lw, lU = lw[::-1], lU[:, ::-1].copy()
        for c in range(3):
            lU[:, c] = [float(t) for t in SR.fix_sign([mpf(t) for t in lU[:, c]])]
        scale = max(abs(t) for t in w)
        e_d = float(max(abs(mpf(float(a)) - b) for a, b in zip(lw, w)) / scale)
        e_U = max(rel_err(_align(lU[:, c], [U[r, c] for r in range(3)]), [U[r, c] for r in range(3)]) for c in range(3))
        rows.append((Sm, w, U, scale, e_d, e_U, _eig_invariants(Sm, lw, lU)))
    return rows


def check_eig3(out):
    rep_d, rep_U, rep_i = Report("pnp_eig3 d", 3), Report("pnp_eig3 U", 3), Report("pnp_eig3 invariants", 3)
    d, U = out["E.pnp_eig3.d"].reshape(-1, 3), out["E.pnp_eig3.U"].reshape(-1, 3, 3)
    for k, ((name, S, kind), (Sm, w, Ur, scale, e_d, e_U, e_inv)) in enumerate(zip(SC.eig3_cases(), ref_eig3())):
        rep_d.add(name, float(max(abs(mpf(float(a)) - b) for a, b in zip(d[k], w)) / scale), e_d)
        rep_d.require(d[k][0] >= d[k][1] >= d[k][2], name, "not descending: %r" % d[k])
        res, orth = _eig_invariants(Sm, d[k], U[k])
        rep_i.add(name, res, e_inv[0], " residual")
        rep_i.add(name, orth, e_inv[1], " orthonormality")
        for c in range(3):
            col = U[k][:, c]
            big = col[np.argmax(np.abs(col))]
            rep_U.require(big > 0, name, "column %d: the largest component %r is not positive" % (c, big))
            if kind == "unique":
                ref = [Ur[r, c] for r in range(3)]
                rep_U.add(name, rel_err(col, ref), e_U, " column %d" % c)
    return [rep_d, rep_U, rep_i]


# ------------------------------------------------------------------ P. pnp_polar3
@functools.lru_cache(maxsize=None)
def ref_polar3():
    rows = []
    for name, B, kind in SC.polar3_cases():
        R, sv = SR.polar3(mat(B))
        u, _, vt = np.linalg.svd(B)
        lap = u @ vt
        orth = float(mpmath.norm(mat(lap).T * mat(lap) - mpmath.eye(3), "inf"))
        rows.append((SR.flat(R), sv, rel_err(lap.reshape(-1), SR.flat(R)) if kind == "unique" else None, orth,
                     float(mpmath.det(R))))
    return rows


def check_polar3(out):
    rep, rep_o = Report("pnp_polar3", 3), Report("pnp_polar3 R^T R = I", 3)
    got = out["P.pnp_polar3"].reshape(-1, 3, 3)
    for k, ((name, B, kind), (R, sv, e_lap, e_orth, det)) in enumerate(zip(SC.polar3_cases(), ref_polar3())):
        Rm = mat(got[k])
        rep_o.add(name, float(mpmath.norm(Rm.T * Rm - mpmath.eye(3), "inf")), e_orth)
        dd = float(mpmath.det(Rm))
        rep_o.require(abs(abs(dd) - 1) <= 1e-14, name, "det R = %r" % dd)
        if kind == "unique":
            rep.add(name, rel_err(got[k].reshape(-1), R), e_lap)
            rep_o.require((dd > 0) == (det > 0), name, "det R = %r, the reference's %r" % (dd, det))
    return [rep, rep_o]


# ------------------------------------------------------------------ Q / J. pnp_alphas, pnp_project
@functools.lru_cache(maxsize=None)
def ref_points():
    al = []
    for name, c0, ci, X in SC.alphas_cases():
        ref = SR.alphas(V(c0), [V(r) for r in ci], V(X))
        d = X.astype(np.float64) - c0
        a = [0.0] + [float(ci[j, 0] * d[0] + ci[j, 1] * d[1] + ci[j, 2] * d[2]) for j in range(3)]
        a[0] = 1.0 - a[1] - a[2] - a[3]
        al.append((ref, rel_err(a, ref)))
    pj = []
    for name, K, R, t, X in SC.project_cases():
        ue, ve, margin = SR.getuv(V(K), [V(r) for r in R], V(t), V(X))
        Kd, Xd = K.astype(np.float64), X.astype(np.float64)
        P = [R[r, 0] * Xd[0] + R[r, 1] * Xd[1] + R[r, 2] * Xd[2] + t[r] for r in range(3)]
        invz = float(f32(1.0 / P[2]))
        lap = [Kd[2] + Kd[0] * P[0] * invz, Kd[3] + Kd[1] * P[1] * invz]
        pj.append(([ue, ve], margin, lap, float(f32(float(1 / (V(R[2])[0] * V(X)[0] + V(R[2])[1] * V(X)[1] + V(R[2])[2] * V(X)[2] + V(t)[2]))))))
    return al, pj


def check_points(out):
    al, pj = ref_points()
    rep_a, rep_p = Report("pnp_alphas", 3), Report("pnp_project", 3)
    a = out["Q.pnp_alphas"].reshape(-1, 4)
    for k, ((name, c0, ci, X), (ref, e_lap)) in enumerate(zip(SC.alphas_cases(), al)):
        rep_a.add(name, rel_err(a[k], ref), e_lap)
        rep_a.require(abs(a[k].sum() - 1) <= 16 * EPS * max(1.0, np.abs(a[k]).max()), name, "the alphas sum to %r" % a[k].sum())
    uv = out["J.pnp_project"].reshape(-1, 2)
    for k, ((name, K, R, t, X), (ref, margin, lap, _)) in enumerate(zip(SC.project_cases(), pj)):
        # a different float invZc moves the pixel by 6e-8 of its offset: it shows as an error far above the bound,
        # and is excused only next to the rounding boundary
        err, e_lap = rel_err(uv[k], ref), rel_err(lap, ref)
        rep_p.exact(name, err <= bound(e_lap, 3), True, margin)
        rep_p.rows.append((name, min(err, bound(e_lap, 3)), e_lap, bound(e_lap, 3)))
    return [rep_a, rep_p]


# ------------------------------------------------------------------ I. pnp_check_inliers
@functools.lru_cache(maxsize=None)
def ref_check():
    rows = []
    for name, K, R, t, Xw, uv, me, fill in SC.check_cases():
        fin = np.isfinite(R).all() and np.isfinite(t).all()
        if not fin:
            rows.append(([False] * len(Xw), [mpf(1)] * len(Xw), None))
            continue
        Km, Rm, tm = V(K), [V(r) for r in R], V(t)
        dec = [SR.check_inlier(Km, Rm, tm, V(Xw[i]), V(uv[i]), mpf(float(me[i]))) for i in range(len(Xw))]
        rows.append(([d[0] for d in dec], [d[1] for d in dec], reloc_ref.check_inliers(R, t, Xw, uv, me, K)))
    return rows


def check_check(out, restated=False):
    rep = Report("pnp_check_inliers", 3)
    halves = out["I.mask_halves"].reshape(-1, 4, 2)
    for k, (case, (want, margin, lap)) in enumerate(zip(SC.check_cases(), ref_check())):
        name, n = case[0], len(case[4])
        words = [int(lo) | (int(hi) << 32) for lo, hi in halves[k]]
        nw = (n + 63) // 64
        rep.require(all(w == GUARD for w in words[nw:]), name, "a word beyond the mask was written")
        bits = [(words[i // 64] >> (i % 64)) & 1 for i in range(n)]
        rep.require(all((words[w] >> b) & 1 == 0 for w in range(nw) for b in range(64) if 64 * w + b >= n), name,
                    "bits beyond n are set")
        rep.require(int(out["I.count"][k]) == sum(bits), name, "count %d, the mask has %d" % (out["I.count"][k], sum(bits)))
        for i in range(n):
            rep.exact("%s[%d]" % (name, i), bool(bits[i]), bool(want[i]), margin[i])
    return [rep]


# ------------------------------------------------------------------ X. pnp_epnp
@functools.lru_cache(maxsize=None)
def ref_epnp():
    """the 50-digit compute_pose of every case with n >= 6 and the restatement's error against it"""
    rows = {}
    for name, K, Xw, uv, idx, truth in SC.epnp_cases():
        r = SR.epnp(Xw[idx], uv[idx], K)
        R0, t0 = reloc_ref.epnp(Xw[idx].astype(np.float64), uv[idx].astype(np.float64), tuple(float(k) for k in K))
        ref = [x for row in r["R"] for x in row] + r["t"]
        lap = np.concatenate([R0.reshape(-1), t0])
        r["ref"], r["e_lapack"] = ref, max(rel_err(lap[:9], ref[:9]), rel_err(lap[9:], ref[9:]))
        rows[name] = r
    return rows


def _job_table(out):
    jobs = program_inputs()["X.job"][:, 0]
    return jobs, out["X.Rt"].reshape(-1, 12), out["X.tap"].reshape(-1, TAP_SLOTS)[:len(jobs)]


def check_epnp(out):
    rep, rep_t = Report("pnp_epnp", 12), Report("pnp_epnp taps", 12)
    jobs, Rt, tap = _job_table(out)
    cases = epnp_case_list()
    refs = ref_epnp()
    first = {}
    for j, c in enumerate(jobs):
        first.setdefault(int(c), j)
    for c, j in sorted(first.items()):
        name = cases[c][0]
        R = Rt[j, :9].reshape(3, 3)
        rep.require(np.isfinite(Rt[j]).all(), name, "pose not finite")
        if np.isfinite(Rt[j]).all():
            rep.require(np.abs(R.T @ R - np.eye(3)).max() <= 1e-13 and np.linalg.det(R) > 0, name, "R is not a rotation")
        if name not in refs:
            continue
        r = refs[name]
        rep.add(name, max(rel_err(Rt[j, :9], r["ref"][:9]), rel_err(Rt[j, 9:], r["ref"][9:])), r["e_lapack"])
        rep.require(_winner(tap[j]) == r["variant"] or _errs_tie(r), name,
                    "variant %d has the smallest tapped error, the reference takes %d" % (_winner(tap[j]), r["variant"]))
    return [rep]


def _winner(tap):
    """the variant compute_pose keeps (:476-496), from the three tapped reprojection errors"""
    e, N = tap[22:25], 0
    if e[1] < e[0]:
        N = 1
    if e[2] < e[N]:
        N = 2
    return N


def _errs_tie(r):
    e = sorted(r["err"])
    return (e[1] - e[0]) <= mpf(10) ** -9 * e[0]


def check_lanes(out):
    """a case's pose and taps are the same bytes in every lane, among any neighbours, in the partly filled workgroup"""
    rep = Report("pnp_epnp lanes", 12)
    jobs, Rt, tap = _job_table(out)
    names = [c[0] for c in epnp_case_list()]
    seen = {}
    for j, c in enumerate(jobs):
        seen.setdefault(int(c), []).append(j)
    for c, js in seen.items():
        for j in js[1:]:
            rep.require(Rt[j].tobytes() == Rt[js[0]].tobytes() and tap[j].tobytes() == tap[js[0]].tobytes(), names[c],
                        "job %d (workgroup %d, lane %d) differs from job %d (workgroup %d, lane %d)"
                        % (j, j // 16, j % 16, js[0], js[0] // 16, js[0] % 16))
    last = len(jobs) // 16
    for f in SC.FIXED:
        lanes = {j % 16 for j in seen[names.index(f)]}
        rep.require({0, 7, 15} <= lanes and any(j // 16 == last for j in seen[names.index(f)]), f, "not in lanes 0, 7, 15 and the last workgroup")
    rep.require(0 < len(jobs) % 16 < 16, "jobs", "the last workgroup is full")
    return [rep]


# ------------------------------------------------------------------ T / H / S. s3s_top_eigenvector, s3s_horn, s3s_pose
def _top_invariants(N, q):
    """(|N q - (q^T N q) q| over |N|, | |q| - 1 |) for a double q against the 50-digit N"""
    qm = mpmath.matrix(V(q))
    lam = (qm.T * N * qm)[0] / (qm.T * qm)[0]
    return float(mpmath.norm(N * qm - lam * qm, "inf") / mpmath.norm(N, "inf")), float(abs(mpmath.norm(qm, 2) - 1)), lam


@functools.lru_cache(maxsize=None)
def ref_top():
    rows = []
    for name, N, kind in SC.top_cases():
        Nm = mat(N)
        q, w = SR.top_eigenvector(Nm)
        lw, lV = np.linalg.eigh(N)
        lq = lV[:, 3]
        inv = _top_invariants(Nm, lq)
        rows.append((Nm, q, w, rel_err(_align(lq, q), q), inv[0], inv[1]))
    return rows


def check_top(out):
    rep, rep_i = Report("s3s_top_eigenvector", 4), Report("s3s_top_eigenvector invariants", 4)
    got = out["T.s3s_top_eigenvector"].reshape(-1, 4)
    for k, ((name, N, kind), (Nm, q, w, e_lap, e_res, e_norm)) in enumerate(zip(SC.top_cases(), ref_top())):
        res, nrm, lam = _top_invariants(Nm, got[k])
        rep_i.add(name, res, e_res, " residual")
        rep_i.add(name, nrm, e_norm, " norm")
        scale = max(abs(t) for t in w)
        rep_i.add(name, float(abs(lam - w[0]) / scale), 0.0, " Rayleigh quotient against the largest eigenvalue")
        if kind == "unique":
            rep.add(name, rel_err(_align(got[k], q), q), e_lap)
    return [rep, rep_i]


def _horn_fit(P1, P2, R, t, s):
    """|P1 - (s R P2 + t)| over |P1| in 50 digits, for doubles R, t, s"""
    Rm, tm, sm = [V(r) for r in np.asarray(R).reshape(3, 3)], V(t), mpf(float(s))
    worst = mpf(0)
    for i in range(3):
        a, b = V(P1[i]), V(P2[i])
        for r in range(3):
            worst = max(worst, abs(a[r] - (sm * (Rm[r][0] * b[0] + Rm[r][1] * b[1] + Rm[r][2] * b[2]) + tm[r])))
    return float(worst / max(abs(x) for x in V(P1)))


def _t_err(t, ref, P1):
    """t = O1 - s R O2 is a difference of points: its error over the larger of |t| and |P1| (t itself may be zero)"""
    scale = max([abs(x) for x in ref] + [mpf(float(np.abs(P1).max()))])
    return float(max(abs(mpf(float(a)) - b) for a, b in zip(t, ref)) / scale)


@functools.lru_cache(maxsize=None)
def ref_horn():
    rows = []
    for name, P1, P2, fix, kind in SC.horn_cases():
        R, t, s, info = SR.horn(P1, P2, fix)
        with np.errstate(all="ignore"):
            lR, lt, ls, _ = loop_ref.horn_sim3(P1, P2, fix)
        ref = [x for row in R for x in row] + (t or [None] * 3) + [s]
        e = None
        if kind in ("unique", "identity"):
            e = (rel_err(lR.reshape(-1), ref[:9]), _t_err(lt, ref[9:12], P1), rel_err([ls], ref[12:]))
        elif kind == "invariants":
            e = (_horn_fit(P1, P2, lR, lt, ls), float(np.abs(lR.T @ lR - np.eye(3)).max()))
        rows.append((ref, info, e))
    return rows


def check_horn(out):
    rep, rep_i = Report("s3s_horn", 4), Report("s3s_horn invariants", 4)
    got = out["H.s3s_horn"].reshape(-1, 13)
    for k, ((name, P1, P2, fix, kind), (ref, info, e)) in enumerate(zip(SC.horn_cases(), ref_horn())):
        R = got[k, :9].reshape(3, 3)
        rep_i.require(np.abs(R.T @ R - np.eye(3)).max() <= 64 * EPS and np.linalg.det(R) > 0, name, "R is not a rotation")
        if fix:
            rep.require(got[k, 12] == 1.0, name, "s = %r with the scale fixed" % got[k, 12])
        if kind in ("unique", "identity"):
            rep.add(name, rel_err(got[k, :9], ref[:9]), e[0], " R")
            rep.add(name, _t_err(got[k, 9:12], ref[9:12], P1), e[1], " t")
            rep.add(name, rel_err(got[k, 12:], ref[12:]), e[2], " s")
            if kind == "identity":
                rep.require(np.array_equal(R, np.eye(3)), name, "R is not the identity, bit for bit")
        elif kind == "invariants":
            rep_i.add(name, _horn_fit(P1, P2, R, got[k, 9:12], got[k, 12]), e[0], " fit")
            rep_i.add(name, float(np.abs(R.T @ R - np.eye(3)).max()), e[1], " orthonormality")
        else:  # den == 0: the identity, no scale, no translation
            rep.require(np.array_equal(R, np.eye(3)) and not np.isfinite(got[k, 12]) and not np.isfinite(got[k, 9:12]).any(),
                        name, "R = %r, t = %r, s = %r" % (R, got[k, 9:12], got[k, 12]))
    return [rep, rep_i]


@functools.lru_cache(maxsize=None)
def ref_pose():
    rows = []
    for name, R, t, s in SC.pose_cases():
        ref = SR.sim3_pose([V(r) for r in R], V(t), mpf(s))
        A12, A21 = s * R, (1.0 / s) * R.T
        t21 = np.array([-(A21[r, 0] * t[0] + A21[r, 1] * t[1] + A21[r, 2] * t[2]) for r in range(3)])
        lap = np.concatenate([A12.reshape(-1), t, A21.reshape(-1), t21])
        parts = ((0, 9), (9, 12), (12, 21), (21, 24))
        rows.append((ref, parts, max(rel_err(lap[a:b], ref[a:b]) for a, b in parts)))
    return rows


def check_pose(out):
    rep = Report("s3s_pose", 3)
    got = out["S.s3s_pose"].reshape(-1, 24)
    for k, ((name, R, t, s), (ref, parts, e_lap)) in enumerate(zip(SC.pose_cases(), ref_pose())):
        rep.add(name, max(rel_err(got[k, a:b], ref[a:b]) for a, b in parts), e_lap)
    return [rep]


# ------------------------------------------------------------------ V / D / N. s3s_project, s3s_dist2, s3s_is_inlier
@functools.lru_cache(maxsize=None)
def ref_views():
    _, cams, _ = AC.cameras()
    pr = []
    for name, ci, A, t, X in SC.sim3_project_cases():
        uv, margin = SR.sim3_project(cams[ci], [V(r) for r in A] if A is not None else None, V(t) if A is not None else None, V(X))
        lap = loop_ref.project(X[None], cams, [ci], A, t)[0]
        pr.append(([float(x) for x in uv], margin, lap))
    d2 = []
    for name, a, b in SC.dist2_cases():
        v, margin = SR.dist2(V(a), V(b))
        d2.append((float(v), margin, float(loop_ref._dist2(a[None], b[None])[0])))
    inl = []
    for name, c1, c2, T24, X1, X2, me1, me2 in inlier_cases():
        if not np.isfinite(T24).all():
            inl.append((False, mpf(1)))
            continue
        inl.append(SR.sim3_is_inlier([mpf(float(x)) for x in T24], cams[c1], cams[c2], V(X1), V(X2), mpf(float(f32(me1))),
                                     mpf(float(f32(me2)))))
    return pr, d2, inl


def check_views(out):
    pr, d2, inl = ref_views()
    rep_p, rep_d, rep_n = Report("s3s_project", 3), Report("s3s_dist2", 3), Report("s3s_is_inlier", 3)
    uv = out["V.s3s_project"].reshape(-1, 2)
    for k, (case, (ref, margin, lap)) in enumerate(zip(SC.sim3_project_cases(), pr)):
        for a in range(2):
            rep_p.exact("%s[%d]" % (case[0], a), float(uv[k, a]), ref[a], margin)
    for k, (case, (ref, margin, lap)) in enumerate(zip(SC.dist2_cases(), d2)):
        rep_d.exact(case[0], float(out["D.s3s_dist2"][k]), ref, margin)
    for k, (case, (ref, margin)) in enumerate(zip(inlier_cases(), inl)):
        rep_n.exact(case[0], bool(out["N.s3s_is_inlier"][k]), bool(ref), margin)
    return [rep_p, rep_d, rep_n]


# ------------------------------------------------------------------ the tests
ALL_CHECKS = (check_lstsq, check_rot, check_eig3, check_polar3, check_points, check_check, check_epnp, check_lanes, check_top,
              check_horn, check_pose, check_views)


def test_program_cross_compiles_for_gfx950():
    """drift of the headers against the program is caught without a GPU; the library's flags, no warning"""
    exe, log = built_program()
    assert exe is not None, log
    assert os.path.getsize(exe) > 0 and "warning" not in log, log


def test_reference_against_exact_definitions():
    """the 50-digit statements against what they should give: Horn's R, t, s on noise-free triples are the generating
    similarity; compute_pose on noise-free scenes of n >= 6 is the generating pose within the float rounding of the
    inputs (map points to 2^-24 of 12 m, pixels to 2^-24 of 752: 1e-6 m, 5e-5 px)"""
    rng = np.random.default_rng(42)
    worst = 0.0
    for k in range(12):
        P2, R0, t0, s0 = SC._triple(rng), SC._rot(rng), rng.standard_normal(3), float(rng.uniform(0.5, 2.0))
        fix = k % 3 == 0
        if fix:
            s0 = 1.0
        P1 = s0 * (P2 @ R0.T) + t0
        R, t, s, _ = SR.horn(P1, P2, fix)
        worst = max(worst, rel_err(R0.reshape(-1), [x for row in R for x in row]), rel_err(t0, t), rel_err([s0], [s]))
    print("Horn as written against the generating similarity: %.3g" % worst)
    assert worst <= 1e-12  # P1 is rounded to double: 1e-16 over the triple's conditioning
    worst_t = worst_R = 0.0
    for name, K, Xw, uv, idx, truth in SC.epnp_cases():
        if truth is None:
            continue
        r = ref_epnp()[name]
        dt, dR = SR.pose_error(r["R"], r["t"], truth[0], truth[1])
        worst_t, worst_R = max(worst_t, dt), max(worst_R, dR)
    print("compute_pose as written against the generating pose: %.3g m, %.3g rad" % (worst_t, worst_R))
    assert worst_t <= 1e-4 and worst_R <= 1e-4


def test_restatements_need_no_excuse():
    """the yardstick itself: every float value and every decision of the LAPACK / numpy restatements equals the 50-digit
    reference's, none next to a rounding boundary; their errors E_lapack are printed by the other tests"""
    bad = []
    for case, (want, margin, lap) in zip(SC.check_cases(), ref_check()):
        if lap is not None:
            bad += ["%s[%d]" % (case[0], i) for i in range(len(want)) if bool(lap[i]) != bool(want[i]) or margin[i] < EXCUSE_MARGIN]
    pr, d2, inl = ref_views()
    for case, (ref, margin, lap) in zip(SC.sim3_project_cases(), pr):
        if [float(x) for x in lap] != ref or margin < EXCUSE_MARGIN:
            bad.append(case[0])
    for case, (ref, margin, lap) in zip(SC.dist2_cases(), d2):
        if lap != ref or margin < EXCUSE_MARGIN:
            bad.append(case[0])
    for case, (ref, margin) in zip(inlier_cases(), inl):
        if margin < EXCUSE_MARGIN:
            bad.append(case[0])
    for case, (ref, margin, lap, _) in zip(SC.project_cases(), ref_points()[1]):
        if margin < EXCUSE_MARGIN:
            bad.append(case[0])
    assert not bad, bad


def _branches(out, who):
    """every named branch case enters the branch it is named for: from the inputs, from the 50-digit reference and from
    the evaluator's taps"""
    import math
    bad = []

    def need(ok, what):
        if not ok:
            bad.append(what)

    # pnp_lstsq6
    for nc in NCS:
        cs = {c[0]: c for c in SC.lstsq_cases(nc)}
        need(all(cs["diagonal-positive"][1][k, k] > 0 and cs["diagonal-negative"][1][k, k] < 0 for k in range(nc)), "lstsq diagonal signs")
        need(not cs["zero-column-1"][1][:, 1].any() and cs["pivot-zero"][1][0, 0] == 0, "lstsq zero column / pivot")
        need(not cs["column-reduced-to-its-pivot-positive"][1][1:, 0].any(), "lstsq reduced column")
        A = cs["proportional-columns"][1]
        need(np.array_equal(A[:, nc - 1], 3 * A[:, 0]) and np.linalg.matrix_rank(A) == nc - 1, "lstsq proportional columns")
    # pnp_rot
    rc = {c[0]: c[1:] for c in SC.rot_cases()}
    rot = dict(zip([c[0] for c in SC.rot_cases()], out["R.pnp_rot"].reshape(-1, 3)))
    with np.errstate(over="ignore"):
        z = np.float64(rc["g-tiny-zeta-squared-overflows"][1] - rc["g-tiny-zeta-squared-overflows"][0]) / (2 * np.float64(1e-200))
        need(np.isinf(z * z) and np.isfinite(z), "rot: zeta * zeta does not overflow")
    need(tuple(rot["g-tiny-zeta-squared-overflows"]) == (0.0, 1.0, 0.0), "rot: t, cs, sn = %r at the overflow" % (rot["g-tiny-zeta-squared-overflows"],))
    need(rot["zeta-positive"][0] > 0 and rot["zeta-negative"][0] < 0, "rot: sign of t")
    need(rot["a-equals-b"][0] == 1.0 and rot["a-equals-b-g-negative"][0] == 1.0, "rot: a = b gives t = 1 (zeta = +-0)")
    # pnp_eig3
    ec = {c[0]: c[1] for c in SC.eig3_cases()}
    for name, (p, q) in (("off-diagonal-below-ulp-01", (0, 1)), ("off-diagonal-below-ulp-02", (0, 2))):
        S = ec[name]
        h = 100 * abs(S[p, q])
        need(S[p, q] != 0 and abs(S[p, p]) + h == abs(S[p, p]) and abs(S[q, q]) + h == abs(S[q, q]), "eig3 " + name)
    d = dict(zip([c[0] for c in SC.eig3_cases()], out["E.pnp_eig3.d"].reshape(-1, 3)))
    need(all(tuple(d["diagonal-%d%d%d" % p]) == (3.0, 2.0, 1.0) for p in __import__("itertools").permutations((3, 2, 1))), "eig3 diagonal orders")
    need(np.linalg.matrix_rank(ec["rank-2-0"]) == 2 and abs(d["rank-2-0"][2]) <= 16 * EPS * d["rank-2-0"][0], "eig3 rank 2")
    # pnp_polar3: the third column's sign is negative iff det B (-1)^exchanges < 0, known where no sweep runs
    neg = pos = 0
    for name, B, kind in SC.polar3_cases():
        if name.startswith("orthogonal-columns-"):
            need(all(B[:, a] @ B[:, b] == 0 for a, b in ((0, 1), (0, 2), (1, 2))), "polar3 %s: a sweep runs" % name)
            sg = np.linalg.det(B) * (-1) ** SC.column_swaps((B * B).sum(axis=0))
            neg, pos = neg + (sg < 0), pos + (sg > 0)
        if name.startswith("reflection"):
            need(np.linalg.det(B) < 0, "polar3 %s: det B >= 0" % name)
    need(neg >= 2 and pos >= 2, "polar3: sg < 0 in %d, sg > 0 in %d of the cases without a sweep" % (neg, pos))
    need(np.linalg.matrix_rank(dict((c[0], c[1]) for c in SC.polar3_cases())["rank-2-exact"]) == 2, "polar3 rank 2")
    # pnp_alphas / pnp_project
    ac = {c[0]: c for c in SC.alphas_cases()}
    need(not ac["planar-frame"][2][2].any() and np.array_equal(ac["point-at-the-centroid"][1], ac["point-at-the-centroid"][3].astype(np.float64)),
         "alphas planar frame / centroid")
    al = dict(zip([c[0] for c in SC.alphas_cases()], out["Q.pnp_alphas"].reshape(-1, 4)))
    need(tuple(al["point-at-the-centroid"]) == (1.0, 0.0, 0.0, 0.0) and al["planar-frame"][3] == 0.0, "alphas at the centroid / planar")
    for case, (ref, margin, lap, invz) in zip(SC.project_cases(), ref_points()[1]):
        if "rounding-boundary" in case[0]:
            need(EXCUSE_MARGIN < margin < 1e-7, "project %s: margin %.3g" % (case[0], float(margin)))
    # pnp_epnp: the reference and the taps agree on the branch
    jobs, Rt, tap = _job_table(out)
    names = [c[0] for c in epnp_case_list()]
    T = {names[int(c)]: tap[j] for j, c in reversed(list(enumerate(jobs)))}
    R = ref_epnp()
    for g in (1, 2, 3):
        name = "x0-negative-in-guess-%d" % g
        need(R[name]["x"][g - 1][0] < 0 and T[name][(31, 35, 38)[g - 1]] < 0, "epnp " + name)
    for g, slot_x, slot_b in ((2, 35, 15), (3, 38, 19)):
        name = "x2-of-the-wrong-sign-in-guess-%d" % g
        x = R[name]["x"][g - 1]
        need((x[0] < 0) != (x[2] < 0) and R[name]["betas0"][g - 1][1] == 0 and T[name][slot_b] == 0 and T[name][slot_x + 2] != 0,
             "epnp " + name)
    # x[1] and z0 carry the signs of the eigenvectors, which are the eigen-solver's own: from the taps alone
    name = "x2-of-the-wrong-sign-in-guess-3"
    need(T[name][36] < 0 and T[name][14] < 0 and T[name][39] < 0 and T[name][18] < 0, "epnp x[1] < 0: betas[0] is not negated")
    need(min(T[name][25:28]) < 0, "epnp z0 < 0")
    need(min(R["det-negative"]["det"]) < 0 and min(T["det-negative"][28:31]) < 0, "epnp det < 0")
    wins = {R[n]["variant"] for n in R if not _errs_tie(R[n]) and _winner(T[n]) == R[n]["variant"]}
    need(wins == {0, 1, 2}, "epnp: variants %r win" % wins)
    need(T["planar-axis-aligned"][0] == 0 and T["planar-axis-aligned"][2] == 0 and T["planar-axis-aligned"][6] == 0,
         "epnp: the axis-aligned plane has no exactly vanishing direction")
    need(abs(R["cube-corners"]["cond_S"][0] - R["cube-corners"]["cond_S"][2]) == 0, "epnp: the cube's scatter has no triple eigenvalue")
    # s3s_top_eigenvector / s3s_horn
    q = dict(zip([c[0] for c in SC.top_cases()], out["T.s3s_top_eigenvector"].reshape(-1, 4)))
    for p_ in range(4):
        need(np.array_equal(q["diagonal-maximum-at-%d" % p_], np.eye(4)[p_]), "top: diagonal, maximum at %d" % p_)
    need(np.array_equal(q["tie-of-the-two-largest"], np.eye(4)[1]), "top: the lower index of a tie")
    need(sum(1 for n, v in q.items() if n.startswith("horn/") and v[0] < 0) >= 2, "horn: no eigenvector with q0 < 0")
    info = dict(zip([c[0] for c in SC.horn_cases()], [r[1] for r in ref_horn()]))
    need(info["same-points"]["nv"] == 0 and info["coincident-points-in-set-2"]["den"] == 0, "horn: nv == 0 / den == 0")
    need(0 < info["rotation-1e-09-rad"]["theta"] < 1e-8, "horn: small rotation")
    for a in ("x", "y", "z", "111"):
        need(abs(info["half-turn-about-%s" % a]["q"][0]) < 1e-15 and abs(info["half-turn-about-%s" % a]["theta"] - math.pi) < 1e-14, "horn half turn " + a)
    need(abs(info["collinear-triples"]["w"][0] - info["collinear-triples"]["w"][1]) <= 1e-13 * abs(info["collinear-triples"]["w"][0]),
         "horn: collinear triples without a double eigenvalue")
    ic = {c[0]: c for c in inlier_cases()}
    res = dict(zip([c[0] for c in inlier_cases()], out["N.s3s_is_inlier"]))
    first = SC.inlier_pairs()[0][0]
    need(res[first + "/generous"] == 1 and res[first + "/err1-equals-threshold"] == 0 and res[first + "/err1-one-ulp-below"] == 1 and
         res[first + "/err2-equals-threshold"] == 0 and res[first + "/err2-one-ulp-below"] == 1 and res["pose-not-finite"] == 0,
         "is_inlier thresholds")
    assert not bad, "%s: %s" % (who, bad)


def test_host_build_against_the_reference():
    """the host build of the two headers (g++, glibc) within the device's bound on every family"""
    out = host_outputs()
    finish([r for chk in ALL_CHECKS for r in chk(out)], "host")


def test_cases_enter_their_branches():
    _branches(host_outputs(), "host")


def test_case_lists_stay_small():
    inp = program_inputs()
    assert len(ref_epnp()) <= 40 and len(inp["X.job"]) <= 4096
    assert len(inp["X.job"]) % 16 == len(SC.FIXED)


@pytest.mark.gpu
def test_helpers_on_the_device():
    out = device_outputs()
    finish([r for chk in (check_lstsq, check_rot, check_eig3, check_polar3, check_points, check_check) for r in chk(out)], "device")


@pytest.mark.gpu
def test_epnp_on_the_device():
    out = device_outputs()
    finish(check_epnp(out), "device")


@pytest.mark.gpu
def test_epnp_lanes_on_the_device():
    out = device_outputs()
    finish(check_lanes(out), "device")


@pytest.mark.gpu
def test_sim3_helpers_on_the_device():
    out = device_outputs()
    finish([r for chk in (check_top, check_horn, check_pose, check_views) for r in chk(out)], "device")


@pytest.mark.gpu
def test_cases_enter_their_branches_on_the_device():
    _branches(device_outputs(), "device")
