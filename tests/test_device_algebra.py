"""The lane functions every optimiser is assembled from (ba_device.h, imu_device.h, cam_project.h, cam_unproject.h),
called directly, one lane per case, and compared with a 50-digit reference (tests/algebra_ref.py) on named cases
(tests/algebra_cases.py).  tests/hip_unit/device_algebra_test.hip evaluates; nothing is compared in C++.

Three statements of every function meet here: *as written* (the reference's formula, branch and float roundings, in
50 digits), *exact* (the mathematical definition) and the CPU oracle's FP64.  The oracle's error against as written,
E_oracle(case), is the yardstick of the device: at most 4 x max(E_oracle(case), 2^-52), max-norm of the difference over
max-norm of the reference output, part by part where an output mixes scales (position, quaternion, bias).  Values the
reference rounds to float are bit-equal to the float of the as-written value unless the 50-digit value lies within
1e-12 of a rounding boundary (at most 2 per 1000).  The GPU tests share one build and one run of the program.

Families: A rotations, B retractions, C cameras, D the visual edge, E the inertial and encoder edges, F triangulation
(null_vector4<4 | 8 | 16>, triangulate_matches_world<2 | 8>), G the block reductions.

Every branch the scenes never enter has a named case, asserted from the inputs, with one exception: the ten-iteration
cap of KB8's SolveTheta.  Its Newton steps converge quadratically for every fisheye polynomial that is monotonic up to
the clamp at pi / 2 (here at most 3 steps), so no input the library may legitimately receive runs ten; the test
asserts that the cap of Radtan's loop is met and that KB8's is not.  The Huber branch is asserted as far as the outputs
show it: the quadratic branch hands back (e, 1) bit for bit, the linear one has rho' < 1 wherever the as-written rho' is
below 1 by more than the bound (one ulp above dsqr both branches give the same doubles).

Found by these tests and fixed: the reference multiplies its float coefficients by int constants in float
(`3 * p[1]` in RadtanCamera::Project's Jacobian, camera_radtan.h:91,95; `9 * k4` ... `3 * k1` in KB8Camera::SolveTheta,
camera_kb8.h:297-303); the oracle did the same, the device multiplied in double.  Shown by cam_project.J/radtan*-k2/...
(every Radtan case: up to 3.8e-12 against a bound of 9e-16, worst ratio 23000) and by cam_unproject/kb8-0/generic-38,
kb8-1/generic-27, kb8-3/generic-23 (ratio up to 2.45: Newton's iterates left the oracle's by an ulp, which tan near
90 degrees magnifies).  cam_project.h and cam_unproject.h now round these products to float.

A deliberately wrong sign (q.w of the trace <= 0 case of R_to_q), tried on a scratch copy, failed R_to_q/... (the 120
degree, 179.999 degree, 100 / 170 degree and generic trace <= 0 cases; the exact half turns have w = 0 and cannot notice),
imu_error/... and imu_linearize/... of the 100 and 170 degree Rij cases, and nothing else.

Measured on an MI355X (E_oracle worst, at which case; median; the device's worst ratio to its bound):

  so3_exp_q           2.3e-16 generic-74                 4.3e-17   0.32
  so3_log_q           2.7e-16 generic-197                6.8e-17   0.25
  so3_Jr_d            3.4e-12 generic-217 (th ~ 1e-5)    9.5e-17   0.25
  so3_JrInv_d         3.4e-07 norm=2pi-1e-9/axis=111     6.3e-17   0.25      (th = pi: against the oracle only)
  quat_to_R           2.6e-16 generic-114                1.0e-16   0.25
  R_to_q              2.6e-16 generic-271                7.5e-17   0.39
  q_mul               2.7e-16 generic-267                7.5e-17   0.25
  q_norm              2.5e-16 generic-146                6.6e-17   0.33
  Jr JrInv = I        worst ratio to its limit 0.083; unit quaternions within 4 ulp
  inc_small_pr        2.9e-16 generic-256                9.9e-17   0.25
  ns_inc              3.2e-16 dphi-norm=7/axis=111       1.0e-16   0.32
  cam_project.J       7.1e-16 kb8-1/generic-40           1.3e-16   0.64      (23000 before the fix)
  cam_unproject (KB8) 6.3e-13 kb8-1/generic-31           7.0e-17   0.48      (2.45 before the fix)
  unproject_pinhole   1.1e-16 kb8-1/generic-15           2.2e-17   0.12
  make_xf             3.6e-16 .../camera-1/depth=200     1.5e-16   0.25
  edge_eval<false>    4.8e-13 .../depth=0.3/stereo       3.3e-15   0.25      .J 9.0e-15 / 2.3e-16 / 0.38
  edge_eval<true>     7.0e-14 .../depth=0.3/stereo       2.1e-16   0.25      .J 7.5e-15 / 3.2e-16 / 0.61
  huber               2.8e-16 generic-63                 0         0.25      (at the edges' chi2 0.35)
  visual_accumulate   against the same sums in FP64                0.25
  imu_error           3.4e-10 residual-below-1e-5/PVR    3.3e-14   0.44
  imu_linearize       3.7e-13 generic-94/PVR             4.9e-16   0.48
  enc_edge_eval       err 1.2e-09 residual-below-1e-5 / 5.6e-14 / 0.44; Ji 9.3e-16 / 2.7e-16 / 0.25; Jj 9.4e-16 / 2.4e-16 / 0.25
  null_vector4<4>     6.5e-16 tri2/generic-25            1.9e-16   0.25      (sign aligned; where the null vector is
  null_vector4<8>     5.2e-16 tri8/generic-2             1.5e-16   0.25       not unique, |A x| <= 64 u s_max instead)
  null_vector4<16>    6.5e-16 tri8/5-observations        1.6e-16   0.25
  triangulate<2>      1.1e-14 (the point)                1.5e-16   0.25      the 111 returns equal as written's, 0 excused
  triangulate<8>      4.4e-15 (the point)                1.6e-16   0.25      the 122 returns equal as written's, 0 excused
  reductions          |sum - exact| over (BS - 1) 2^-53 sum|v|: block_sum<1..27> 0.003 .. 0.005, block_sum_bs<.,64> 0.023
                      and 0.037, block_sum_bs<.,256> 0.003 and 0.005, block_sum_lds<28,64> 0.046, <28,256> 0.004; every
                      thread the same bits, second call = first call on the same data, integers exact
  excused float values: 0 of 2414 (cam_project, with and without J), 0 of 650 (Radtan cam_unproject), 0 of 1776 visual
  residuals, for the oracle and for the device alike; part 1 + part 2 = part 0 and edge_eval<true> with = without
  cam_xf, bit for bit

As written against exact (asserted unless marked):

  so3_exp_q 1.0e-28, so3_Jr_d 4.2e-17, so3_JrInv_d 1.4e-23, so3_log_q 3.9e-17 (M_PI is a double), R_to_q 8.9e-16
  (the inputs' own orthonormality), inc_small_pr 9.5e-29, imu_error 1.1e-37
  Jacobians against central differences at h = 1e-15: cam_project (pinhole, regular KB8) 9.8e-30, the visual edge
  3.8e-31, imu_linearize 1.7e-31; KB8 cam_unproject, projected back, 1.1e-17 of the pixel's offset
  null_vector4: A^T A x = s_4^2 x for the vector of mpmath.svd_r, 6.4e-51 (the DLT point itself is the reference's
  estimator, 'not the best method', and is not compared with the scene's)
  not asserted, the reference's own (CAMERA_GAPS): Radtan Jacobian 0.32 of its max-norm (0.073 in the edge) because fd2
  starts at k[2]; KB8's pinhole branch 4.0e-10; Radtan cam_unproject 3.5e-6 of the pixel's offset after its ten
  Gauss-Newton steps; KB8 cam_unproject with thetad clamped at pi / 2 or a field angle beyond 90 degrees: the mirrored
  point
"""
import atexit
import functools
import math
import os
import shutil
import struct
import subprocess
import tempfile

import numpy as np
import pytest
from mpmath import mpf

from tests import algebra_cases as AC
from tests import algebra_ref as AR
from vieo_slam_amd.ba_types import NAVSTATE_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
U = 2.0 ** -53           # unit roundoff of a double
EPS = 2.0 ** -52
EXCUSE_MARGIN = 1e-12    # a float rounding may differ only this close (relative) to a rounding boundary
EXCUSE_CAP = 2e-3        # at most 2 per 1000 values of a family


# ------------------------------------------------------------------ the stand-alone program and its files
def write_blob(path, arrays):
    """magic, table of contents, flat little-endian arrays (see device_algebra_test.hip)"""
    items = []
    for name, a in arrays.items():
        a = np.ascontiguousarray(a)
        if a.dtype == np.float64:
            items.append((name, 0, a.astype("<f8").reshape(-1)))
        elif a.dtype == np.int32:
            items.append((name, 1, a.astype("<i4").reshape(-1)))
        else:
            raise TypeError((name, a.dtype))
    off = 16 + 56 * len(items)
    toc = b""
    for name, dt, a in items:
        assert len(name) < 32, name
        toc += struct.pack("<32siiqq", name.encode(), dt, 0, a.size, off)
        off += a.nbytes
    with open(path, "wb") as f:
        f.write(b"VIEOALG1" + struct.pack("<ii", len(items), 0) + toc)
        for _, _, a in items:
            f.write(a.tobytes())


def read_blob(path):
    raw = open(path, "rb").read()
    assert raw[:8] == b"VIEOALG1"
    n, = struct.unpack_from("<i", raw, 8)
    out = {}
    for k in range(n):
        name, dt, _, count, off = struct.unpack_from("<32siiqq", raw, 16 + 56 * k)
        out[name.rstrip(b"\0").decode()] = np.frombuffer(raw, "<f8" if dt == 0 else "<i4", count, off).copy()
    return out


def hipcc_flags():
    """the library's code generation: FLAGS of vieo_slam_amd/build.py without -fPIC; VIEO_POSE_DPP64 stays undefined"""
    from vieo_slam_amd import build as B
    return [f for f in B.FLAGS if f != "-fPIC"], B.HIPCC


@functools.lru_cache(maxsize=None)
def built_program():
    """(path, None) of the program built into a temporary directory, or (None, compiler output); once per session"""
    flags, hipcc = hipcc_flags()
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc") or hipcc
    d = tempfile.mkdtemp(prefix="device_algebra_")
    atexit.register(shutil.rmtree, d, True)
    exe = os.path.join(d, "device_algebra_test")
    r = subprocess.run([hipcc] + flags + ["-o", exe, os.path.join(HERE, "hip_unit", "device_algebra_test.hip")],
                       capture_output=True, text=True)
    if r.returncode != 0:
        return None, r.stdout + r.stderr
    return exe, None


def cam_tables():
    names, cams, sizes = AC.cameras()
    f = np.zeros((len(cams), 25))
    i = np.zeros((len(cams), 2), np.int32)
    for k, c in enumerate(cams):
        f[k, 0:4] = [float(c["fx"]), float(c["fy"]), float(c["cx"]), float(c["cy"])]
        f[k, 4] = AC.camera_bf(c)
        f[k, 5:14], f[k, 14:17] = c["Rcb"], c["tcb"]
        f[k, 17:25] = c["dist"].astype(np.float64)
        i[k] = [int(c["model"]), int(c["num_k"]) if c["model"] == 1 else 0]
    return f, i


def _stack(cases, k):
    return np.array([c[k] for c in cases], np.float64)


@functools.lru_cache(maxsize=None)
def program_inputs():
    rv, qs, ms, qp, rq = AC.rotvec_cases(), AC.quat_cases(), AC.matrix_cases(), AC.quat_pair_cases(), AC.raw_quat_cases()
    pi, si = AC.pose_inc_cases(), AC.state_inc_cases()
    pc, uc, hc = AC.project_cases(), AC.unproject_cases(), AC.pinhole_unproject_cases()
    cf, ci = cam_tables()
    ic, ec = AC.imu_cases(), AC.enc_cases()
    vc, hcs = AC.visual_cases(), AC.huber_cases()
    pool, _ = AC.reduction_pool()
    inp = {
        "A.rotvec": _stack(rv, 1), "A.quat": _stack(qs, 1), "A.mat": _stack(ms, 1), "A.mul_a": _stack(qp, 1),
        "A.mul_b": _stack(qp, 2), "A.raw_quat": _stack(rq, 1),
        "B.pose": _stack(pi, 1), "B.pose_inc": _stack(pi, 2), "B.state": _stack(si, 1), "B.state_inc": _stack(si, 2),
        "B.bias_inc": _stack(si, 3),
        "C.cam_f64": cf, "C.cam_i32": ci,
        "C.project_cam": np.array([c[1] for c in pc], np.int32), "C.project_P": _stack(pc, 2),
        "C.unproject_cam": np.array([c[1] for c in uc], np.int32), "C.unproject_uv": _stack(uc, 2),
        "C.pinhole_cam": np.array([c[1] for c in hc], np.int32), "C.pinhole_uv": _stack(hc, 2),
        "D.cam0": np.array([c[1] for c in vc], np.int32), "D.rig": np.array([c[2] for c in vc], np.int32),
        "D.pose": _stack(vc, 3), "D.obs": _stack(vc, 4), "D.flags": np.array([c[5] for c in vc], np.int32),
        "D.delta": _stack(vc, 6), "D.huber_e": _stack(hcs, 1), "D.huber_delta": _stack(hcs, 2),
        "D.huber_dsqr": _stack(hcs, 3),
        "E.imu_meas": _stack(ic, 1), "E.imu_gw": _stack(ic, 2), "E.imu_si": _stack(ic, 3), "E.imu_sj": _stack(ic, 4),
        "E.imu_idR": np.array([c[5] for c in ic], np.int32),
        "E.enc_si": _stack(ec, 1), "E.enc_sj": _stack(ec, 2), "E.enc_meas": _stack(ec, 3), "E.enc_qbe": _stack(ec, 4),
        "E.enc_pbe": _stack(ec, 5),
        "G.pool": pool,
    }
    _, nul = tri_case_lists()
    for M in NULL_M:
        inp["F.null%d_A" % M] = np.array([c[1] for c in nul[M]], np.float64)
    for N in TRI_N:
        si, sf, af, ai = _tri_inputs(N)
        inp.update({"F.tri%d_slot_i32" % N: si, "F.tri%d_slot_f64" % N: sf, "F.tri%d_arg_f64" % N: af, "F.tri%d_arg_i32" % N: ai})
    return inp


@functools.lru_cache(maxsize=None)
def device_run():
    """("ok", outputs) or ("failed", message): the program is built once, fed once and run once; a failure is cached
    and every test reports it without starting the program again"""
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


# ------------------------------------------------------------------ errors and bounds
def rel_err(x, ref):
    """max-norm of the difference over the max-norm of the reference output (absolute where the reference is zero)"""
    d = max(abs(mpf(float(a)) - b) for a, b in zip(x, ref))
    m = max(abs(b) for b in ref)
    return float(d / m) if m != 0 else float(d)


def parts_err(x, ref, parts):
    """an output made of parts of different scale (position, quaternion, bias ...): the worst part"""
    return max(rel_err(x[a:b], ref[a:b]) for a, b in parts)


class Table:
    """one function on one case list: names, the as-written outputs (lists of mpf), the oracle's outputs (arrays),
    the oracle's error per case and the parts an output is made of"""

    def __init__(self, fn, names, ref, orc, parts=None):
        self.fn, self.names, self.ref, self.orc = fn, names, ref, orc
        self.parts = parts or [(0, len(ref[0]))]
        self.e_oracle = [parts_err(o, r, self.parts) for o, r in zip(orc, ref)]

    def bound(self, k):
        return 4 * max(self.e_oracle[k], EPS)

    def check_device(self, dev, skip=(), indexed=False):
        """device against as written, case by case: at most 4 x max(E_oracle(case), 2^-52); the failures as messages,
        or as (case index, message) pairs"""
        dev = np.asarray(dev).reshape(len(self.names), -1)
        worst, bad = 0.0, []
        for k, name in enumerate(self.names):
            if name in skip:
                continue
            e = parts_err(dev[k], self.ref[k], self.parts)
            ratio = e / self.bound(k)
            worst = max(worst, ratio)
            if not ratio <= 1.0:
                bad.append((k, "%s/%s: error %.3g, bound %.3g (E_oracle %.3g)" % (self.fn, name, e, self.bound(k),
                                                                                   self.e_oracle[k])))
        print("%-22s device worst ratio to its bound %.3f over %d cases" % (self.fn, worst, len(self.names)))
        return bad if indexed else [m for _, m in bad]

    def figures(self):
        e = np.array(self.e_oracle)
        return "%-22s E_oracle worst %.3g (%s), median %.3g" % (self.fn, e.max(), self.names[int(e.argmax())],
                                                                 float(np.median(e)))


def ceiling_check(t, ceil, indexed=False):
    """reference against oracle: E_oracle(case) <= ceil(case), a ceiling reasoned from the function's conditioning"""
    bad = []
    for k, name in enumerate(t.names):
        c = ceil(k) if callable(ceil) else ceil
        if c is not None and not t.e_oracle[k] <= c:
            bad.append((k, "%s/%s: oracle against as written %.3g, ceiling %.3g" % (t.fn, name, t.e_oracle[k], c)))
    print(t.figures())
    return bad if indexed else [m for _, m in bad]


# ------------------------------------------------------------------ A. rotations
@functools.lru_cache(maxsize=None)
def tables_A():
    from tests import oracle_lib
    O = oracle_lib.load()
    rv, qs, ms, qp, rq = AC.rotvec_cases(), AC.quat_cases(), AC.matrix_cases(), AC.quat_pair_cases(), AC.raw_quat_cases()
    n_rv, n_q = [c[0] for c in rv], [c[0] for c in qs]
    T = {}
    T["so3_exp_q"] = Table("so3_exp_q", n_rv, [AR.so3_exp_aw(AR.V(c[1])) for c in rv], [O.so3_exp(c[1]) for c in rv])
    T["so3_Jr_d"] = Table("so3_Jr_d", n_rv, [AR.so3_Jr_aw(AR.V(c[1])) for c in rv],
                          [O.so3_jr(c[1]).reshape(-1) for c in rv])
    T["so3_JrInv_d"] = Table("so3_JrInv_d", n_rv, [AR.so3_JrInv_aw(AR.V(c[1])) for c in rv],
                             [O.so3_jr(c[1], inverse=True).reshape(-1) for c in rv])
    T["so3_log_q"] = Table("so3_log_q", n_q, [AR.so3_log_aw(AR.V(c[1])) for c in qs], [O.so3_log(c[1]) for c in qs])
    T["quat_to_R"] = Table("quat_to_R", n_q, [AR.quat_to_R(AR.V(c[1])) for c in qs], [O.quat_to_R(c[1]) for c in qs])
    T["R_to_q"] = Table("R_to_q", [c[0] for c in ms], [AR.R_to_q_aw(AR.V(c[1])) for c in ms],
                        [O.R_to_quat(c[1]) for c in ms])
    T["q_mul"] = Table("q_mul", [c[0] for c in qp], [AR.q_mul(AR.V(c[1]), AR.V(c[2])) for c in qp],
                       [O.quat_mul(c[1], c[2]) for c in qp])
    T["q_norm"] = Table("q_norm", [c[0] for c in rq], [AR.q_norm(AR.V(c[1])) for c in rq],
                        [O.quat_normalize(c[1]) for c in rq])
    return T


def _theta(w):
    return float(np.linalg.norm(w))


JRINV_AT_PI = tuple("norm=pi/axis=%s" % a for a, _ in AC.AXES)   # sin(th) is about 1e-16 there: oracle only


def test_rotations_reference_against_oracle():
    """E_oracle ceilings.  A handful of roundings on O(1) terms: 16 u.  so3_Jr_d: (1 - cos th) / th carries cos's
    rounding u divided by th, so 16 u (1 + 1 / th) above 1e-5.  so3_JrInv_d: (1 + cos th) th / (2 sin th) carries it
    times th / (2 |sin th|), so 16 u (1 + th / |sin th|); at th = pi the ceiling is void."""
    T, bad = tables_A(), []
    rv = AC.rotvec_cases()
    for fn in ("so3_exp_q", "so3_log_q", "quat_to_R", "R_to_q", "q_mul", "q_norm"):
        bad += ceiling_check(T[fn], 16 * U)
    bad += ceiling_check(T["so3_Jr_d"], lambda k: 16 * U * (1 + (1 / _theta(rv[k][1]) if _theta(rv[k][1]) >= 1e-5 else 0)))

    def jrinv(k):
        th = _theta(rv[k][1])
        if rv[k][0] in JRINV_AT_PI:
            return None
        return 16 * U * (1 + (th / abs(math.sin(th)) if th >= 1e-5 else 0))
    bad += ceiling_check(T["so3_JrInv_d"], jrinv)
    assert not bad, "\n".join(bad)


def test_rotations_as_written_against_exact():
    """The closed forms of so3_extra.h against the definitions.  Each small-angle branch drops a term below 1e-20 at
    th < 1e-5 (th^4 / 3840 in exp, th^3 / 24 and th^4 / 720 in the Jacobians, 2/5 w^5 in log), and log's M_PI is a
    double (relative 4e-17): every gap must stay below 1e-15, relative to the output's max-norm.  R_to_q is exact when
    its matrix is a rotation; the inputs are orthonormal to a few u, so quat_to_R(R_to_q(R)) = R to 1e-14."""
    bad, worst = [], {}

    def see(fn, name, aw, ex, tol):
        m = max(abs(b) for b in ex)
        g = float(max(abs(a - b) for a, b in zip(aw, ex)) / (m if m != 0 else 1))
        worst[fn] = max(worst.get(fn, 0.0), g)
        if not g <= tol:
            bad.append("%s/%s: as written against exact %.3g" % (fn, name, g))
    for name, w in AC.rotvec_cases():
        w = AR.V(w)
        see("so3_exp_q", name, AR.so3_exp_aw(w), AR.so3_exp_ex(w), 1e-15)
        see("so3_Jr_d", name, AR.so3_Jr_aw(w), AR.so3_Jr_ex(w), 1e-15)
        see("so3_JrInv_d", name, AR.so3_JrInv_aw(w), AR.so3_JrInv_ex(w), 1e-15)
    for name, q in AC.quat_cases():
        q = AR.q_norm(AR.V(q))      # the definitions speak of unit quaternions
        see("so3_log_q", name, AR.so3_log_aw(q), AR.so3_log_ex(q), 1e-15)
    for name, R in AC.matrix_cases():
        R = AR.V(R)
        see("R_to_q", name, AR.quat_to_R(AR.R_to_q_aw(R)), R, 1e-14)
    for fn, g in worst.items():
        print("%-22s as written against exact, worst gap %.3g" % (fn, g))
    assert not bad, "\n".join(bad)


def test_rotation_cases_enter_every_branch():
    """asserted from the inputs themselves, so that a reseeded or edited case list cannot lose a branch"""
    ms = [AR.R_to_q_branch(AR.V(c[1])) for c in AC.matrix_cases()]
    assert {"trace", 0, 1, 2} <= set(ms)
    names = [c[0] for c in AC.matrix_cases()]
    assert ms[names.index("trace-zero-120deg-about-111")] != "trace"     # trace = 0 exactly takes the else
    assert ms[names.index("half-turn-about-110")] == 0 and ms[names.index("half-turn-about-011")] == 1   # the ties
    lb = {}
    for name, q in AC.quat_cases():
        lb.setdefault(AR.so3_log_branch(AR.V(q)), []).append(name)
    assert {"n<eps", "w>0", "w<=0", "atan"} <= set(lb)
    assert "w=0/axis=x" in lb["w<=0"] and any(q[0] < -0.1 for _, q in AC.quat_cases())
    th = np.array([_theta(c[1]) for c in AC.rotvec_cases()])
    assert (th == 0).any() and ((th > 0) & (th < 1e-5)).any() and (th == AC.BELOW).any() and (th == 1e-5).any()
    assert (th == AC.ABOVE).any() and (th > 6).any()
    for cases, col in ((AC.pose_inc_cases(), 2), (AC.state_inc_cases(), 2)):
        th = np.array([_theta(c[col][-3:]) for c in cases])
        assert ((th < 1e-5).any() and (th >= 1e-5).any() and (th == 0).any())


@pytest.mark.gpu
def test_rotations_on_the_device():
    out, T, bad = device_outputs(), tables_A(), []
    for fn in ("so3_exp_q", "so3_Jr_d", "so3_log_q", "quat_to_R", "R_to_q", "q_mul", "q_norm"):
        bad += T[fn].check_device(out["A." + fn])
    bad += T["so3_JrInv_d"].check_device(out["A.so3_JrInv_d"], skip=JRINV_AT_PI)
    t = T["so3_JrInv_d"]
    dev = out["A.so3_JrInv_d"].reshape(len(t.names), 9)
    for k, name in enumerate(t.names):          # th = pi: against the oracle only
        if name in JRINV_AT_PI:
            e = float(np.abs(dev[k] - t.orc[k]).max() / np.abs(t.orc[k]).max())
            if not e <= 4 * EPS:
                bad.append("so3_JrInv_d/%s: device against oracle %.3g" % (name, e))
    # unit quaternions to 4 ulp
    for fn in ("so3_exp_q", "R_to_q", "q_norm"):
        q = out["A." + fn].reshape(-1, 4)
        n2 = [float(abs(sum(mpf(float(c)) ** 2 for c in r) - 1)) for r in q]      # |q|^2 - 1 = 2 (|q| - 1)
        k = int(np.argmax(n2))
        if not n2[k] / 2 <= 4 * EPS:
            bad.append("%s/%s: norm off by %.3g" % (fn, T[fn].names[k], n2[k] / 2))
    # Jr JrInv = I for th <= 3: each factor within its own bound, so the product (formed here without rounding) is
    # within |dJr| |JrInv| + |Jr| |dJrInv| summed over the three terms of a row
    rv = AC.rotvec_cases()
    jr, jri = out["A.so3_Jr_d"].reshape(-1, 9), out["A.so3_JrInv_d"].reshape(-1, 9)
    worst = 0.0
    for k, (name, w) in enumerate(rv):
        if _theta(w) > 3:
            continue
        Pm = AR.mm3(AR.V(jr[k]), AR.V(jri[k]))
        d = float(max(abs(a - b) for a, b in zip(Pm, AR.eye3())))
        ma, mb = float(max(abs(t) for t in T["so3_Jr_d"].ref[k])), float(max(abs(t) for t in t.ref[k]))
        lim = 3 * ma * mb * (T["so3_Jr_d"].bound(k) + t.bound(k)) + 1e-20
        worst = max(worst, d / lim)
        if not d <= lim:
            bad.append("Jr JrInv = I/%s: off by %.3g, limit %.3g" % (name, d, lim))
    print("Jr JrInv = I           worst ratio to its limit %.3f" % worst)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------ B. retractions
POSE_PARTS = [(0, 3), (3, 7)]
STATE_PARTS = [(0, 3), (3, 6), (6, 10), (10, 13), (13, 16), (16, 19), (19, 22)]


def _navstate(s):
    n = np.zeros(1, NAVSTATE_DTYPE)
    n["p"], n["v"], n["q"], n["bg"], n["ba"], n["dbg"], n["dba"] = s[0:3], s[3:6], s[6:10], s[10:13], s[13:16], s[16:19], s[19:22]
    return n


def _state_of(n):
    n = n[0] if n.shape else n
    return np.concatenate([n["p"], n["v"], n["q"], n["bg"], n["ba"], n["dbg"], n["dba"]])


@functools.lru_cache(maxsize=None)
def tables_B():
    from tests import oracle_lib
    O = oracle_lib.load()
    pi, si = AC.pose_inc_cases(), AC.state_inc_cases()
    ref, orc = [], []
    for name, s, d in pi:
        p, q = AR.inc_small_pr_aw(AR.V(s[0:3]), AR.V(s[3:7]), AR.V(d))
        ref.append(p + q)
        st = np.zeros(22)
        st[0:3], st[6:10] = s[0:3], s[3:7]
        o = O.lba_navstate_inc(_navstate(st)[0], np.concatenate([d, np.zeros(9)]))
        orc.append(np.concatenate([o["p"], o["q"]]))
    T = {"inc_small_pr": Table("inc_small_pr", [c[0] for c in pi], ref, orc, POSE_PARTS)}
    ref, orc = [], []
    for name, s, d9, db in si:
        p, v, q, dbg, dba = AR.ns_inc_aw(AR.V(s[0:3]), AR.V(s[3:6]), AR.V(s[6:10]), AR.V(s[16:19]), AR.V(s[19:22]),
                                         AR.V(d9), AR.V(db))
        ref.append(p + v + q + AR.V(s[10:16]) + dbg + dba)
        orc.append(_state_of(O.navstate_inc(_navstate(s), d9, db)))
    T["ns_inc"] = Table("ns_inc", [c[0] for c in si], ref, orc, STATE_PARTS)
    return T


def test_retractions_reference_against_oracle():
    """p + R dp is three products and three sums on a position of up to 10 m: 16 u of the part's max-norm; the
    quaternion is a product of unit quaternions and two normalisations: 16 u; a bias sum is one rounding"""
    T, bad = tables_B(), []
    for fn in T:
        bad += ceiling_check(T[fn], 16 * U)
    assert not bad, "\n".join(bad)


def test_retractions_as_written_against_exact():
    """NavState::IncSmall uses SO3ex::exp, whose small-angle branch is exact to 1e-20 (above)"""
    worst = 0.0
    for name, s, d in AC.pose_inc_cases():
        a = AR.inc_small_pr_aw(AR.V(s[0:3]), AR.V(s[3:7]), AR.V(d))
        b = AR.inc_small_pr_ex(AR.V(s[0:3]), AR.V(s[3:7]), AR.V(d))
        g = float(max(abs(x - y) for x, y in zip(a[0] + a[1], b[0] + b[1])))
        worst = max(worst, g)
        assert g <= 1e-15, (name, g)
    print("inc_small_pr           as written against exact, worst gap %.3g" % worst)


@pytest.mark.gpu
def test_retractions_on_the_device():
    out, T, bad = device_outputs(), tables_B(), []
    bad += T["inc_small_pr"].check_device(out["B.inc_small_pr"])
    bad += T["ns_inc"].check_device(out["B.ns_inc"])
    for fn, sl in (("inc_small_pr", slice(3, 7)), ("ns_inc", slice(6, 10))):
        q = out["B." + fn].reshape(len(T[fn].names), -1)[:, sl]
        n2 = [float(abs(sum(mpf(float(c)) ** 2 for c in r) - 1)) for r in q]
        k = int(np.argmax(n2))
        if not n2[k] / 2 <= 4 * EPS:
            bad.append("%s/%s: norm off by %.3g" % (fn, T[fn].names[k], n2[k] / 2))
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------ C. cameras
def _cam_dicts():
    names, cams, _ = AC.cameras()
    return [{"model": int(c["model"]), "num_k": int(c["num_k"]), "fx": c["fx"], "fy": c["fy"], "cx": c["cx"],
             "cy": c["cy"], "dist": c["dist"]} for c in cams], cams, names


class FloatTable:
    """values the reference rounds to float: bit-equal to the float of the as-written value, unless the 50-digit value
    lies within 1e-12 (relative) of a point at which a rounding on its way changes"""

    def __init__(self, fn, names, ref, margin):
        self.fn, self.names, self.ref, self.margin = fn, names, ref, margin

    def check(self, got, who):
        got = np.asarray(got).reshape(len(self.names), -1)
        bad, excused, total = [], 0, 0
        for k, name in enumerate(self.names):
            for j, r in enumerate(self.ref[k]):
                total += 1
                if float(r) == float(got[k, j]):
                    continue
                if self.margin[k] <= EXCUSE_MARGIN:
                    excused += 1
                else:
                    bad.append("%s/%s[%d]: %s gives %r, as written %r (margin %.3g)" % (
                        self.fn, name, j, who, float(got[k, j]), float(r), float(self.margin[k])))
        print("%-22s %s: %d of %d float values excused" % (self.fn, who, excused, total))
        if excused > EXCUSE_CAP * total:
            bad.append("%s: %d of %d values excused, over 2 per 1000" % (self.fn, excused, total))
        return bad, excused, total


@functools.lru_cache(maxsize=None)
def tables_C():
    from tests import oracle_lib
    O = oracle_lib.load()
    cd, cams, _ = _cam_dicts()
    pc, uc, hc = AC.project_cases(), AC.unproject_cases(), AC.pinhole_unproject_cases()
    T = {}
    uv_ref, uv_margin, J_ref, uv_or, J_or = [], [], [], [], []
    for name, ci, Pc in pc:
        P = AR.V(Pc)
        uv, J = AR.cam_project_aw(cd[ci], P)
        raw, _ = AR.cam_project_aw(cd[ci], P, rounded=False)
        uv_ref.append(uv), J_ref.append(J), uv_margin.append(min(AR.f32_margin(t) for t in raw))
        a, b = O.cam_project(cams[ci], Pc)
        uv_or.append(a.astype(np.float64)), J_or.append(b.reshape(-1).copy())
    names = [c[0] for c in pc]
    T["cam_project.uv"] = FloatTable("cam_project.uv", names, uv_ref, uv_margin)
    T["cam_project.uv.oracle"] = np.array(uv_or)
    T["cam_project.J"] = Table("cam_project.J", names, J_ref, J_or)
    # cam_unproject: Radtan hands back floats, KB8 and the pinhole doubles
    rn, rref, rmargin, ror, kn, kref, kor, kinfo = [], [], [], [], [], [], [], []
    for name, ci, uv in uc:
        info = {}
        P = AR.cam_unproject_aw(cd[ci], mpf(float(uv[0])), mpf(float(uv[1])), info)
        o = O.cam_unproject(cams[ci], uv)
        if cd[ci]["model"] == 1:
            rn.append(name), rref.append(P[:2]), ror.append(o[:2].copy())
            rmargin.append(min([AR.f32_margin(t) for t in info["unrounded"]] + [info["min_inner_margin"]]))
        else:
            kn.append(name), kref.append(P), kor.append(o.copy()), kinfo.append(info)
    T["cam_unproject.radtan"] = FloatTable("cam_unproject.radtan", rn, rref, rmargin)
    T["cam_unproject.radtan.oracle"] = np.array(ror)
    T["cam_unproject.radtan.rows"] = [k for k, c in enumerate(uc) if cd[c[1]]["model"] == 1]
    T["cam_unproject"] = Table("cam_unproject", kn, kref, kor)
    T["cam_unproject.info"] = kinfo
    T["cam_unproject.rows"] = [k for k, c in enumerate(uc) if cd[c[1]]["model"] != 1]
    T["unproject_pinhole"] = Table("unproject_pinhole", [c[0] for c in hc],
                                   [AR.unproject_pinhole_aw(cd[c[1]], mpf(float(c[2][0])), mpf(float(c[2][1]))) for c in hc],
                                   [np.array([(c[2][0] - float(cams[c[1]]["cx"])) / float(cams[c[1]]["fx"]),
                                              (c[2][1] - float(cams[c[1]]["cy"])) / float(cams[c[1]]["fy"]), 1.0]) for c in hc])
    return T


def test_cameras_reference_against_oracle():
    """The image point and Radtan's unprojection are floats: the oracle gives the float of the as-written value, bar
    excused values (at most 2 per 1000, or the case list is to be reseeded).  Jacobians: sums and products of O(1)
    terms under the max-norm: 64 u.  KB8 unprojection ends in tan(theta), whose relative condition is
    theta (1 + tan^2) / tan: 64 u (1 + that).  (unproject_pinhole has no hook of its own: its 'oracle' is the same two
    divisions in FP64, correctly rounded: u.)"""
    T, bad = tables_C(), []
    bad += T["cam_project.uv"].check(T["cam_project.uv.oracle"], "oracle")[0]
    bad += T["cam_unproject.radtan"].check(T["cam_unproject.radtan.oracle"], "oracle")[0]
    bad += ceiling_check(T["cam_project.J"], 64 * U)
    info = T["cam_unproject.info"]

    def kb8(k):
        th = float(info[k].get("theta", 0.0))
        return 64 * U * (1 + (th * (1 + math.tan(th) ** 2) / abs(math.tan(th)) if th else 0))
    bad += ceiling_check(T["cam_unproject"], kb8)
    bad += ceiling_check(T["unproject_pinhole"], 2 * U)
    assert not bad, "\n".join(bad)


# as written and exact differ by the reference's own choice: printed, not asserted
CAMERA_GAPS = {
    "radtan": "camera_radtan.h:84-90: fd2 starts at k[2], so the radial terms of k[0], k[1] are missing from d(u,v)/dP",
    "kb8-pinhole-branch": "camera_kb8.h:149-151: r <= 1e-5f degenerates to the pinhole Jacobian (gap of order theta^2)",
    "radtan-unproject": "camera_radtan.h:147-169: Gauss-Newton on float image points with that Jacobian, 10 iterations",
    "kb8-unproject-clamp": "camera_kb8.h:175: thetad is clamped to pi/2, beyond which UnProject is no inverse",
    "kb8-unproject-beyond-90deg": "camera_kb8.h:184: on the plane z = 1 a field angle beyond pi/2 is tan's mirrored point",
}


def test_cameras_as_written_against_exact():
    """cam_project's Jacobian against central differences (h = 1e-15 under 50 digits) of the unrounded projection: the
    pinhole and the regular KB8 branch are the derivative itself and must agree to 1e-25 of the max-norm; the entries of
    CAMERA_GAPS are the reference's own and are only printed.  KB8's UnProject solves its equation by Newton steps to
    |fix| < 1e-8, which leaves an error of the order of fix^2: projecting the result gives the pixel back to 1e-12 of
    the pixel's offset from the principal point, unless thetad was clamped."""
    cd, cams, _ = _cam_dicts()
    pc = AC.project_cases()
    gaps, bad = {}, []
    per_model = {}
    for k, (name, ci, Pc) in enumerate(pc):
        m = cd[ci]["model"]
        key = (ci, name.split("/")[1].split("-")[0])
        if per_model.get(key, 0) >= 4:      # a few of each kind per camera: the derivative costs 6 projections
            continue
        per_model[key] = per_model.get(key, 0) + 1
        P = AR.V(Pc)
        J, Jx = AR.cam_project_aw(cd[ci], P)[1], AR.cam_project_J_ex(cd[ci], P)
        g = float(max(abs(a - b) for a, b in zip(J, Jx)) / max(abs(b) for b in Jx))
        if m == 1:
            gaps["radtan"] = max(gaps.get("radtan", 0.0), g)
        elif m == 2 and AR.kb8_project_branch(cd[ci], P) == "pinhole":
            gaps["kb8-pinhole-branch"] = max(gaps.get("kb8-pinhole-branch", 0.0), g)
        else:
            gaps["asserted"] = max(gaps.get("asserted", 0.0), g)
            if not g <= 1e-25:
                bad.append("cam_project.J/%s: as written against exact %.3g" % (name, g))
    for name, ci, uv in AC.unproject_cases():
        if cd[ci]["model"] == 0:
            continue
        info = {}
        u, v = mpf(float(uv[0])), mpf(float(uv[1]))
        P = AR.cam_unproject_aw(cd[ci], u, v, info)
        back = AR.cam_project_ex(cd[ci], P)
        off = max(abs(u - mpf(float(cams[ci]["cx"]))), abs(v - mpf(float(cams[ci]["cy"]))), mpf(1))
        g = float(max(abs(back[0] - u), abs(back[1] - v)) / off)
        if cd[ci]["model"] == 1:
            gaps["radtan-unproject"] = max(gaps.get("radtan-unproject", 0.0), g)
        elif info["clamped"]:
            gaps["kb8-unproject-clamp"] = max(gaps.get("kb8-unproject-clamp", 0.0), g)
        elif info.get("theta", 0) > AR.mp.pi / 2:
            gaps["kb8-unproject-beyond-90deg"] = max(gaps.get("kb8-unproject-beyond-90deg", 0.0), g)
        else:
            gaps["kb8-unproject"] = max(gaps.get("kb8-unproject", 0.0), g)
            if not g <= 1e-12:
                bad.append("cam_unproject/%s: projecting the result misses the pixel by %.3g of its offset" % (name, g))
    for k, g in gaps.items():
        print("cameras                as written against exact, %s: worst gap %.3g%s" % (
            k, g, "  [not asserted: %s]" % CAMERA_GAPS[k] if k in CAMERA_GAPS else ""))
    assert set(CAMERA_GAPS) <= set(gaps)
    assert not bad, "\n".join(bad)


def test_camera_cases_enter_every_branch():
    cd, cams, names = _cam_dicts()
    assert sorted({(c["model"], c["num_k"]) for c in cd if c["model"] == 1}) == [(1, 2), (1, 3), (1, 4), (1, 6)]
    br = {AR.kb8_project_branch(cd[ci], AR.V(P)) for _, ci, P in AC.project_cases() if cd[ci]["model"] == 2}
    assert br == {"regular", "pinhole"}
    assert any(cd[ci]["model"] == 2 and P[2] < 0 for _, ci, P in AC.project_cases())
    info = tables_C()["cam_unproject.info"]
    assert {"solve", "axis"} <= {i.get("branch") for i in info} and any(i.get("clamped") for i in info)
    # the ten-iteration cap: Radtan's loop meets it (the float image point keeps |e| above 1e-8); KB8's Newton steps
    # converge quadratically on every camera a calibration can yield and stop after at most a handful, so its cap is
    # beyond what a legitimate input reaches
    rad = [AR.cam_unproject_aw(cd[ci], mpf(float(uv[0])), mpf(float(uv[1])), d) and d["iterations"]
           for _, ci, uv in AC.unproject_cases() if cd[ci]["model"] == 1 for d in [{}]]
    assert max(rad) == AR.MAX_ITER
    assert 1 < max(i.get("iterations", 0) for i in info) < AR.MAX_ITER


@pytest.mark.gpu
def test_cameras_on_the_device():
    out, T, bad = device_outputs(), tables_C(), []
    b1, e1, n1 = T["cam_project.uv"].check(out["C.cam_project.uv"], "device")
    b2, e2, n2 = T["cam_project.uv"].check(out["C.cam_project.uv_with_J"], "device, with J")
    un = out["C.cam_unproject"].reshape(-1, 3)
    rows = T["cam_unproject.radtan.rows"]
    b3, e3, n3 = T["cam_unproject.radtan"].check(un[rows][:, :2], "device")
    bad += b1 + b2 + b3
    if e1 + e2 + e3 > EXCUSE_CAP * (n1 + n2 + n3):
        bad.append("cameras: %d of %d float values excused, over 2 per 1000" % (e1 + e2 + e3, n1 + n2 + n3))
    if not (un[:, 2] == 1.0).all():
        bad.append("cam_unproject: z is not 1 on the plane")
    bad += T["cam_project.J"].check_device(out["C.cam_project.J"])
    bad += T["cam_unproject"].check_device(un[T["cam_unproject.rows"]])
    bad += T["unproject_pinhole"].check_device(out["C.unproject_pinhole"])
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------ D. the visual edge
XF_PARTS = [(0, 9), (9, 12), (12, 21)]
EDGE_PARTS = [(0, 1), (1, 4), (4, 7)]          # chi2, err, Pc


def _obs_record(ob, flags):
    from vieo_slam_amd.ba_types import POSE_OBS_DTYPE
    o = np.zeros(1, POSE_OBS_DTYPE)
    o["Xw"], o["u"], o["v"], o["ur"], o["inv_sigma2"], o["flags"] = ob[0:3], ob[3], ob[4], ob[5], ob[6], flags
    return o


def _cam_dict_full(c):
    return {"model": int(c["model"]), "num_k": int(c["num_k"]), "fx": c["fx"], "fy": c["fy"], "cx": c["cx"], "cy": c["cy"],
            "dist": c["dist"], "Rcb": c["Rcb"], "tcb": c["tcb"]}


def _rows(J, stereo):
    return list(J[:18 if stereo else 12])


@functools.lru_cache(maxsize=None)
def tables_D():
    from tests import oracle_lib
    O = oracle_lib.load()
    _, cams, _ = AC.cameras()
    vc = AC.visual_cases()
    names = [c[0] for c in vc]
    R = {k: ([], []) for k in ("xf", "edge", "J", "edge_mc", "J_mc")}
    margin, margin_mc, stereo_of = [], [], []
    for name, c0, rig, pose, ob, flags, delta in vc:
        p, q, Xw, stereo = AR.V(pose[0:3]), AR.V(pose[3:7]), AR.V(ob[0:3]), ob[5] >= 0
        stereo_of.append(bool(stereo))
        for key, cam, bf, mlist in (("", cams[c0], AC.camera_bf(cams[c0]), margin),
                                    ("_mc", cams[rig + ((flags >> 8) & 3)], None, margin_mc)):
            bf = AC.camera_bf(cam) if bf is None else bf
            cd = _cam_dict_full(cam)
            chi2, err, Pc, J, raw = AR.edge_eval_aw(cd, mpf(bf), p, q, Xw, AR.V(ob[3:6]), mpf(float(ob[6])))
            oxf, oerr, oPc, ochi2, oJ = O.pose_edge_eval_cam(cam, bf, pose[0:3], pose[3:7], _obs_record(ob, flags))
            if key == "":
                Rcw, tcw, Rwb = AR.edge_xf_aw(cd, p, q)
                R["xf"][0].append(Rcw + tcw + Rwb), R["xf"][1].append(oxf)
            R["edge" + key][0].append([chi2] + err + Pc), R["edge" + key][1].append(np.concatenate([[ochi2], oerr, oPc]))
            R["J" + key][0].append(_rows(J, stereo)), R["J" + key][1].append(np.array(_rows(oJ.reshape(-1), stereo)))
            mlist.append(float(min(AR.f32_margin(t) for t in raw)))
    T = {"make_xf": Table("make_xf", names, *R["xf"], XF_PARTS),
         "edge_eval<false>": Table("edge_eval<false>", names, *R["edge"], EDGE_PARTS),
         "edge_eval<false>.J": Table("edge_eval<false>.J", names, *R["J"]),
         "edge_eval<true>": Table("edge_eval<true>", names, *R["edge_mc"], EDGE_PARTS),
         "edge_eval<true>.J": Table("edge_eval<true>.J", names, *R["J_mc"]),
         "margin": margin, "margin_mc": margin_mc, "stereo": stereo_of}
    hc = AC.huber_cases()
    ref = [AR.huber_aw(mpf(float(c[1])), mpf(float(c[2])), mpf(float(c[3]))) for c in hc]
    T["huber"] = Table("huber", [c[0] for c in hc], [r[0] for r in ref], [O.huber(c[1], c[2], c[3])[:2] for c in hc], [(0, 1), (1, 2)])
    T["huber.branch"] = [r[1] for r in ref]
    return T


def _excusing(failures, margins):
    """failures: (case index, message) pairs.  A residual that differs because the float image point rounds the other
    way is excused when the unrounded image point lies within 1e-12 of that rounding's boundary; returns (the messages
    that remain, number excused)"""
    keep = [m for k, m in failures if not margins[k] <= EXCUSE_MARGIN]
    return keep, len(failures) - len(keep)


def test_visual_edge_reference_against_oracle():
    """E_oracle ceilings.  Rcw, Rwb: sums of three products of O(1) terms, 16 u; tcw = -(Rcw p) + tcb with |p| up to
    10 m: 16 u |p| / |tcw|.  Pc = Rcw Xw + tcw cancels terms of size |Xw| + |p| down to the depth: 16 u S / |Pc|.  The
    residual is a difference of floats, exact in FP64: the oracle must give the as-written value to u of the
    residual's size (bit for bit but for the stereo row's bf / z), or the image point's rounding is excused.  chi2:
    8 u.  The Jacobian is the camera's (64 u) times Pc's conditioning."""
    T, bad = tables_D(), []
    vc = AC.visual_cases()

    def S(k):
        return 3 * (np.abs(vc[k][4][0:3]).max() + np.abs(vc[k][3][0:3]).max() + 1)
    xf = T["make_xf"]
    bad += ceiling_check(xf, lambda k: 16 * U * max(1.0, S(k) / float(max(abs(t) for t in xf.ref[k][9:12]))))
    n_exc = 0
    for fn, mk in (("edge_eval<false>", "margin"), ("edge_eval<true>", "margin_mc")):
        t = T[fn]

        def edge_ceiling(k, t=t):
            Pc = float(max(abs(x) for x in t.ref[k][4:7]))
            err = float(max(abs(x) for x in t.ref[k][1:4]))
            z = abs(float(t.ref[k][6]))
            # the stereo row holds bf / z: Pc's error reaches it through bf / z^2
            e_err = (4 * U * 800 + 50 * 16 * U * S(k) / (z * z)) / err if err else 4 * U * 800
            return max(16 * U * S(k) / Pc, e_err, 2 * e_err + 8 * U)
        b, n = _excusing(ceiling_check(t, edge_ceiling, indexed=True), T[mk])
        bad += b
        n_exc += n
        tj = T[fn + ".J"]
        bad += ceiling_check(tj, lambda k, t=t: 64 * U * (1 + 4 * S(k) / abs(float(t.ref[k][6]))))
    assert n_exc <= EXCUSE_CAP * 2 * 3 * len(vc), n_exc
    bad += ceiling_check(T["huber"], 4 * U)
    assert not bad, "\n".join(bad)


def test_visual_edge_as_written_against_exact():
    """linearizeOplus (g2otypes.h:439-498) against central differences (h = 1e-15 under 50 digits) of the residual with
    the unrounded image point, over p + R dp and R Exp(dphi).  With a pinhole or a regular-branch KB8 camera it is the
    derivative itself: 1e-20 of its max-norm.  With a Radtan camera it inherits camera_radtan.h:84-90 (printed)."""
    _, cams, _ = AC.cameras()
    vc = AC.visual_cases()
    worst, gap_rad, done = 0.0, 0.0, 0
    for name, c0, rig, pose, ob, flags, delta in vc:
        if done >= 32 or "depth=5" not in name or "Rcb=body" not in name:
            continue
        done += 1
        cam = cams[rig + ((flags >> 8) & 3)]
        cd, bf = _cam_dict_full(cam), mpf(AC.camera_bf(cam))
        p, q, Xw, obs, info = AR.V(pose[0:3]), AR.q_norm(AR.V(pose[3:7])), AR.V(ob[0:3]), AR.V(ob[3:6]), mpf(float(ob[6]))
        stereo = ob[5] >= 0
        J = AR.edge_eval_aw(cd, bf, p, q, Xw, obs, info)[3]

        def resid(d):
            pp, qq = AR.inc_small_pr_ex(p, q, d)
            Rcw, tcw, _ = AR.edge_xf_aw(cd, pp, qq)
            a = AR.mv3(Rcw, Xw)
            Pc = [a[k] + tcw[k] for k in range(3)]
            uv = AR.cam_project_ex(cd, Pc)
            return [obs[0] - uv[0], obs[1] - uv[1], obs[2] - (uv[0] - bf / Pc[2])]
        g = 0
        for c in range(6):
            d = [mpf(0)] * 6
            d[c] = AR.H_FD
            ep = resid(d)
            d[c] = -AR.H_FD
            em = resid(d)
            for r in range(3 if stereo else 2):
                g = max(g, abs((ep[r] - em[r]) / (2 * AR.H_FD) - J[r * 6 + c]))
        g = float(g / max(abs(t) for t in J[:12]))
        if cd["model"] == 1:
            gap_rad = max(gap_rad, g)
        else:
            worst = max(worst, g)
            assert g <= 1e-20, (name, g)
    assert done >= 16 and gap_rad > 0
    print("edge_eval.J            as written against central differences, worst gap %.3g over %d cases" % (worst, done))
    print("edge_eval.J            with a Radtan camera: gap %.3g  [not asserted: %s]" % (gap_rad, CAMERA_GAPS["radtan"]))


def test_visual_edge_cases_enter_every_branch():
    _, cams, names = _cam_dicts()
    vc = AC.visual_cases()
    assert {(c[5] >> 8) & 3 for c in vc} == {0, 1, 2, 3} and {c[4][5] >= 0 for c in vc} == {True, False}
    assert {bool((cams[c[1]]["Rcb"] == np.eye(3).reshape(-1)).all()) for c in vc} == {True, False}
    assert {int(cams[c[2] + ((c[5] >> 8) & 3)]["model"]) for c in vc} == {0, 1, 2}
    z = [float(r[6]) for r in tables_D()["edge_eval<false>"].ref]
    assert min(z) < 0.35 and max(z) > 150 and min(z) > 0.05
    hb = tables_D()["huber.branch"]
    hn = [c[0] for c in AC.huber_cases()]
    assert hb[hn.index("mono/e=dsqr")] == "quadratic" and hb[hn.index("mono/e-above-dsqr")] == "linear"
    assert hb[hn.index("stereo/e-below-dsqr")] == "quadratic" and {"quadratic", "linear"} == set(hb)


@pytest.mark.gpu
def test_visual_edge_on_the_device():
    out, T, bad = device_outputs(), tables_D(), []
    n = len(T["make_xf"].names)
    bits = lambda a: np.ascontiguousarray(a).view(np.int64)
    ee, vj, ef = out["D.edge_error"].reshape(n, 7), out["D.visual_jacobian"].reshape(n, 18), out["D.edge_eval<false>"].reshape(n, 25)
    et0, et1, etn = out["D.edge_eval<true>"].reshape(n, 25), out["D.edge_eval<true>.table"].reshape(n, 25), out["D.edge_eval<true>.no_J"].reshape(n, 7)
    if not (bits(et0) == bits(et1)).all():
        bad.append("edge_eval<true>/%s: differs with and without cam_xf" % T["make_xf"].names[int(np.flatnonzero((bits(et0) != bits(et1)).any(1))[0])])
    if not ((bits(ef[:, :7]) == bits(ee)).all() and (bits(ef[:, 7:]) == bits(vj)).all()):
        bad.append("edge_eval<false> is not edge_error followed by visual_jacobian")
    if not (bits(etn) == bits(et0[:, :7])).all():
        bad.append("edge_eval<true>: the residual differs with and without J")
    bad += T["make_xf"].check_device(out["D.make_xf"])
    n_exc = 0
    for fn, dev, mk in (("edge_eval<false>", ef, "margin"), ("edge_eval<true>", et0, "margin_mc")):
        b, k = _excusing(T[fn].check_device(dev[:, :7], indexed=True), T[mk])
        bad += b
        n_exc += k
        tj = T[fn + ".J"]
        worst = 0.0
        for k, name in enumerate(tj.names):           # a monocular edge has two rows
            m = 18 if T["stereo"][k] else 12
            e = rel_err(dev[k, 7:7 + m], tj.ref[k])
            worst = max(worst, e / tj.bound(k))
            if not e <= tj.bound(k):
                bad.append("%s/%s: error %.3g, bound %.3g (E_oracle %.3g)" % (tj.fn, name, e, tj.bound(k), tj.e_oracle[k]))
        print("%-22s device worst ratio to its bound %.3f over %d cases" % (tj.fn, worst, len(tj.names)))
    print("visual edge            %d residuals excused" % n_exc)
    if n_exc > EXCUSE_CAP * 2 * 3 * n:
        bad.append("visual edge: %d residuals excused, over 2 per 1000" % n_exc)
    # Huber: on the named widths, and on each edge's own chi2; the branch is the reference's
    bad += T["huber"].check_device(out["D.huber"])
    # the branch: the quadratic one hands back (e, 1) bit for bit; the linear one shows in rho' < 1 wherever the
    # as-written rho' is further below 1 than the bound (one ulp above dsqr it rounds to 1 in FP64 as well)
    hc = AC.huber_cases()
    for k, (nm, r) in enumerate(zip(T["huber"].names, out["D.huber"].reshape(-1, 2))):
        if T["huber.branch"][k] == "quadratic":
            if not (r[0] == hc[k][1] and r[1] == 1.0):
                bad.append("huber/%s: not the quadratic branch's (e, 1)" % nm)
        elif 1 - T["huber"].ref[k][1] > 4 * EPS and not r[1] < 1.0:
            bad.append("huber/%s: not the linear branch" % nm)
    vc = AC.visual_cases()
    hub, acc = out["D.edge_huber"].reshape(n, 2), out["D.visual_accumulate"].reshape(n, 27)
    worst_h = worst_a = 0.0
    for k, c in enumerate(vc):
        d = float(c[6])
        ref, _ = AR.huber_aw(mpf(float(ef[k, 0])), mpf(d), mpf(d * d))
        worst_h = max(worst_h, max(rel_err(hub[k, 0:1], ref[0:1]), rel_err(hub[k, 1:2], ref[1:2])) / (4 * EPS))
        # visual_accumulate on the device's own J, err and rho': against the 50-digit sums, with the same sums in
        # FP64 (Python floats) as the yardstick
        J, err, info, r1, st = ef[k, 7:], ef[k, 1:4], float(c[4][6]), float(hub[k, 1]), T["stereo"][k]
        ra = AR.accumulate_aw(AR.V(J), AR.V(err), mpf(info), mpf(r1), st)
        w, rows = r1 * info, 3 if st else 2
        fa = [sum(J[r * 6 + a] * w * J[r * 6 + b] for r in range(rows)) for a in range(6) for b in range(a, 6)]
        fa += [sum(J[r * 6 + a] * (-(info * err[r]) * r1) for r in range(rows)) for a in range(6)]
        e_or = max(rel_err(fa[:21], ra[:21]), rel_err(fa[21:], ra[21:]))
        e = max(rel_err(acc[k, :21], ra[:21]), rel_err(acc[k, 21:], ra[21:]))
        worst_a = max(worst_a, e / (4 * max(e_or, EPS)))
        if not e <= 4 * max(e_or, EPS):
            bad.append("visual_accumulate/%s: error %.3g, bound %.3g" % (c[0], e, 4 * max(e_or, EPS)))
    if not worst_h <= 1:
        bad.append("huber at the edges' chi2: worst ratio %.3g" % worst_h)
    print("huber (edge chi2)      device worst ratio to its bound %.3f" % worst_h)
    print("visual_accumulate      device worst ratio to its bound %.3f" % worst_a)
    assert not bad, "\n".join(bad[:60])


# ------------------------------------------------------------------ E. inertial and encoder edges
ERR_PARTS = [(0, 3), (3, 6), (6, 9)]
M_FIELDS = (("dt", 0, 1), ("Rij", 1, 10), ("vij", 10, 13), ("pij", 13, 16), ("JgR", 16, 25), ("Jgv", 25, 34),
            ("Jav", 34, 43), ("Jgp", 43, 52), ("Jap", 52, 61))


def _meas_dict(M):
    d = {k: AR.V(M[a:b]) for k, a, b in M_FIELDS}
    d["dt"] = d["dt"][0]
    return d


def _state_dict(s):
    return {"p": AR.V(s[0:3]), "v": AR.V(s[3:6]), "q": AR.V(s[6:10]), "dbg": AR.V(s[16:19]), "dba": AR.V(s[19:22])}


def _prv_to_device(J):
    """the oracle's PRV columns (PR_i, PR_j, V_i, V_j, Bias_i) in the device's order (state j, state i, Bias_i)"""
    J = np.asarray(J).reshape(9, 24)
    return np.hstack([J[:, 6:12], J[:, 15:18], J[:, 0:6], J[:, 12:15], J[:, 18:24]])


def _imu_scale(M, gw, si, sj):
    """the sizes of the terms that cancel in the position / velocity rows, and th / |sin th| of the rotation residual"""
    dt = M[0]
    a = np.abs
    Sp = a(sj[0:3]).max() + a(si[0:3]).max() + a(si[3:6]).max() * dt + a(gw).max() * dt * dt / 2 + a(M[13:16]).max() + 1
    Sv = a(sj[3:6]).max() + a(si[3:6]).max() + a(gw).max() * dt + a(M[10:13]).max() + 1
    return 3 * Sp, 3 * Sv


@functools.lru_cache(maxsize=None)
def tables_E():
    from tests import oracle_lib
    from vieo_slam_amd.ba_types import LBA_IMU_EDGE_DTYPE, LBA_VIO_PARAMS_DTYPE, VIO_FRAME_DTYPE
    O = oracle_lib.load()
    ic, ec = AC.imu_cases(), AC.enc_cases()
    names, eref, jref, eor, jor = [], [], [], [], []
    for name, M, gw, si, sj, idR in ic:
        md, a, b = _meas_dict(M), _state_dict(si), _state_dict(sj)
        e = AR.imu_error_aw(md, AR.V(gw), a, b, idR)
        names.append(name), eref.append(e), jref.append(AR.imu_linearize_aw(md, AR.V(gw), a, b, e, idR))
        if idR == 6:
            F = np.zeros(1, VIO_FRAME_DTYPE)
            for k, lo, hi in M_FIELDS:
                F["imu"][k] = M[lo] if k == "dt" else M[lo:hi]
            F["gw"] = gw
            oe, Ji, Jj, JB = O.imu_edge_eval(F, _navstate(si), _navstate(sj))
            eor.append(oe.copy()), jor.append(np.hstack([Jj, Ji, JB]).reshape(-1))
        else:
            prm, ed = np.zeros(1, LBA_VIO_PARAMS_DTYPE), np.zeros(1, LBA_IMU_EDGE_DTYPE)
            prm["gw"] = gw
            for k, lo, hi in M_FIELDS:
                ed["imu"][k] = M[lo] if k == "dt" else M[lo:hi]
            oe, J = O.lba_imu_edge_eval(prm, ed, _navstate(si)[0], _navstate(sj)[0])
            eor.append(oe[:9].copy()), jor.append(_prv_to_device(J).reshape(-1))
    T = {"imu_error": Table("imu_error", names, eref, eor, ERR_PARTS), "imu_linearize": Table("imu_linearize", names, jref, jor)}
    names, eref, iref, jref, eor, ior, jor = [], [], [], [], [], [], []
    for name, si, sj, meas, qbe, pbe in ec:
        e, Ji, Jj = AR.enc_edge_aw(_state_dict(si), _state_dict(sj), AR.V(meas), AR.V(qbe), AR.V(pbe))
        oe, oi, oj = O.enc_edge_eval(_navstate(si)[0], _navstate(sj)[0], meas, qbe, pbe)
        names.append(name), eref.append(e), iref.append(Ji), jref.append(Jj)
        eor.append(oe.copy()), ior.append(oi.reshape(-1).copy()), jor.append(oj.reshape(-1).copy())
    T["enc_edge_eval.err"] = Table("enc_edge_eval.err", names, eref, eor, [(0, 3), (3, 6)])
    T["enc_edge_eval.Ji"] = Table("enc_edge_eval.Ji", names, iref, ior)
    T["enc_edge_eval.Jj"] = Table("enc_edge_eval.Jj", names, jref, jor)
    return T


def test_inertial_reference_against_oracle():
    """E_oracle ceilings.  The position and velocity rows are differences of terms of size S (positions up to 10 m,
    v dt, g dt^2 / 2, the measurement) that cancel to a residual of millimetres: an absolute error of 32 u S, so
    32 u S / |row| relative.  The rotation row is the log of a chain of six unit-quaternion products and
    normalisations, each good to a few u absolutely: 64 u / |e_R| (times pi near a half turn).  The Jacobian holds
    those differences (hat of the rows), identity blocks and JrInv(e_R), whose own ceiling is 16 u (1 + th / |sin th|):
    64 u (S + th / |sin th|) of its max-norm, which is at least 1."""
    T, bad = tables_E(), []
    ic = AC.imu_cases()

    def err_ceiling(k):
        _, M, gw, si, sj, idR = ic[k]
        Sp, Sv = _imu_scale(M, gw, si, sj)
        r = [float(max(abs(t) for t in T["imu_error"].ref[k][a:a + 3])) for a in (0, idR, 9 - idR)]
        return max(32 * U * Sp / r[0] if r[0] else 32 * U * Sp, 64 * U * 4 / r[1] if r[1] else 64 * U * 4,
                   32 * U * Sv / r[2] if r[2] else 32 * U * Sv)

    def J_ceiling(k):
        _, M, gw, si, sj, idR = ic[k]
        Sp, Sv = _imu_scale(M, gw, si, sj)
        th = float(AR.norm3(T["imu_error"].ref[k][idR:idR + 3]))
        return 64 * U * (max(Sp, Sv) + (th / abs(math.sin(th)) if th >= 1e-5 else 1))
    bad += ceiling_check(T["imu_error"], err_ceiling)
    bad += ceiling_check(T["imu_linearize"], J_ceiling)
    ec = AC.enc_cases()

    def enc_err(k):
        r = T["enc_edge_eval.err"].ref[k]
        rR, rp = float(max(abs(t) for t in r[0:3])), float(max(abs(t) for t in r[3:6]))
        S = 3 * (np.abs(ec[k][1][0:3]).max() + np.abs(ec[k][2][0:3]).max() + 1)
        return max(64 * U * 4 / rR, 32 * U * S / rp)

    def enc_J(k):
        th = float(AR.norm3(T["enc_edge_eval.err"].ref[k][0:3]))
        return 64 * U * (4 + (th / abs(math.sin(th)) if th >= 1e-5 else 1))
    bad += ceiling_check(T["enc_edge_eval.err"], enc_err)
    bad += ceiling_check(T["enc_edge_eval.Ji"], enc_J)
    bad += ceiling_check(T["enc_edge_eval.Jj"], enc_J)
    assert not bad, "\n".join(bad)


def _retract(s, d, idR):
    """NavState::IncSmall in exact arithmetic: columns p, then R at idR and V at 9 - idR"""
    idV = 9 - idR
    Rd = AR.mv3(AR.quat_to_R(s["q"]), d[0:3])
    return {"p": [s["p"][k] + Rd[k] for k in range(3)], "v": [s["v"][k] + d[idV + k] for k in range(3)],
            "q": AR.q_norm(AR.q_mul(s["q"], AR.so3_exp_ex(d[idR:idR + 3]))), "dbg": s["dbg"], "dba": s["dba"]}


def test_inertial_as_written_against_exact():
    """The residual with SO3ex's closed forms against the one with the exact exp and log (1e-15, as for the rotations),
    and linearizeOplus against central differences of the exact residual at h = 1e-15 under 50 digits, over the
    retraction the vertices use (p + R dp, R Exp(dphi), v + dv, bias + db).  Every block of g2otypes.h:814-859 is the
    first-order derivative, so the whole Jacobian must agree to 1e-20 of its max-norm; at most 32 cases."""
    ic = AC.imu_cases()
    worst_e = worst_J = 0.0
    done = 0
    for k, (name, M, gw, si, sj, idR) in enumerate(ic):
        md, g, a, b = _meas_dict(M), AR.V(gw), _state_dict(si), _state_dict(sj)
        a["q"], b["q"] = AR.q_norm(a["q"]), AR.q_norm(b["q"])     # the definitions speak of rotations
        e_aw, e_ex = AR.imu_error_aw(md, g, a, b, idR), AR.imu_error_ex(md, g, a, b, idR)
        ge = float(max(abs(x - y) for x, y in zip(e_aw, e_ex)))
        worst_e = max(worst_e, ge)
        assert ge <= 1e-15, (name, ge)
        if done >= 32 or not (name.startswith(("dt=0.5/bias-1e-3", "residual", "clean")) or name.startswith("generic-1/")):
            continue
        done += 1
        J = AR.imu_linearize_aw(md, g, a, b, e_ex, idR)
        h = AR.H_FD
        gJ = 0
        for c in range(24):
            es = []
            for sgn in (1, -1):
                d = [mpf(0)] * 9
                aa, bb = a, b
                if c < 9:
                    d[c] = sgn * h
                    bb = _retract(b, d, idR)
                elif c < 18:
                    d[c - 9] = sgn * h
                    aa = _retract(a, d, idR)
                else:
                    aa = dict(a)
                    key, j = ("dbg", c - 18) if c < 21 else ("dba", c - 21)
                    aa[key] = list(a[key])
                    aa[key][j] += sgn * h
                es.append(AR.imu_error_ex(md, g, aa, bb, idR))
            for r in range(9):
                gJ = max(gJ, abs((es[0][r] - es[1][r]) / (2 * h) - J[r * 24 + c]))
        gJ = float(gJ / max(abs(t) for t in J))
        worst_J = max(worst_J, gJ)
        assert gJ <= 1e-20, (name, gJ)
    assert done >= 8
    print("imu_error              as written against exact, worst gap %.3g" % worst_e)
    print("imu_linearize          as written against central differences, worst gap %.3g over %d cases" % (worst_J, done))


def test_inertial_cases_enter_every_branch():
    ic = AC.imu_cases()
    br = {AR.R_to_q_branch(AR.V(c[1][1:10])) for c in ic}
    assert {"trace", 0, 1, 2} <= br                              # Rij of 100 and 170 degrees about each axis
    T = tables_E()["imu_error"]
    th = {n: float(AR.norm3(r[c[5]:c[5] + 3])) for n, r, c in zip(T.names, T.ref, ic)}
    assert th["clean-measurement/PVR"] == 0 and all(t == 0 for t in T.ref[T.names.index("clean-measurement/PRV")])
    assert 0 < th["residual-below-1e-5/PVR"] < 1e-5 and 2.9 < th["residual-3rad/PRV"] < 3.1
    assert {c[1][0] for c in ic} == {0.05, 0.5} and {c[5] for c in ic} == {3, 6}
    assert any(not c[3][16:22].any() for c in ic) and any(c[3][16:22].all() for c in ic)


@pytest.mark.gpu
def test_inertial_and_encoder_edges_on_the_device():
    out, T, bad = device_outputs(), tables_E(), []
    bad += T["imu_error"].check_device(out["E.imu_error"])
    bad += T["imu_linearize"].check_device(out["E.imu_linearize"])
    for a, b in (("E.imu_error", "E.imu_error.parts"), ("E.imu_linearize", "E.imu_linearize.parts")):
        if not (out[a].view(np.int64) == out[b].view(np.int64)).all():      # part 1 + part 2 bit-equal to part 0
            k = int(np.flatnonzero(out[a].view(np.int64) != out[b].view(np.int64))[0])
            bad.append("%s/%s: part 1 then part 2 differs from part 0" % (a, T["imu_error"].names[k // (out[a].size // len(T["imu_error"].names))]))
    for fn in ("enc_edge_eval.err", "enc_edge_eval.Ji", "enc_edge_eval.Jj"):
        bad += T[fn].check_device(out["E." + fn])
    if not (out["E.enc_edge_eval.err"].view(np.int64) == out["E.enc_edge_eval.err_only"].view(np.int64)).all():
        bad.append("enc_edge_eval: the residual differs with and without Jacobians")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------ F. triangulation
NULL_M = (4, 8, 16)       # null_vector4<M>: two observations, the fisheye stage's four cameras, eight observations
TRI_N = (2, 8)            # triangulate_matches_world<N> as tri_search.hip launches it


def _oracle():
    from tests import oracle_lib
    return oracle_lib.load()


@functools.lru_cache(maxsize=None)
def tri_case_lists():
    O = _oracle()
    return {N: AC.tri_cases(N, O) for N in TRI_N}, {M: AC.null_cases(M, O) for M in NULL_M}


def _align(x, ref):
    """a singular vector has no sign of its own: the one nearer the reference"""
    x = np.asarray(x, np.float64)
    return -x if sum(float(a) * float(b) for a, b in zip(x, ref)) < 0 else x


def _residual(A, x):
    """|A x| over the largest singular value, for a unit x: what a null vector is measured by when it is not unique"""
    Ax = [sum(mpf(float(A[r][c])) * mpf(float(x[c])) for c in range(4)) for r in range(len(A))]
    return AR.mpmath.sqrt(sum(t * t for t in Ax))


def _tri_inputs(N):
    tc = tri_case_lists()[0][N]
    si = np.zeros((len(tc), N, 2), np.int32)
    sf = np.zeros((len(tc), N, 19))
    af, ai = np.zeros((len(tc), 4)), np.zeros(len(tc), np.int32)
    for k, (name, slots, thresh, just, x3d) in enumerate(tc):
        for j, (on, ci, T, nP, u, v, s2, ur, bf) in enumerate(slots):
            si[k, j] = [int(on), ci]
            sf[k, j] = np.concatenate([np.asarray(T, np.float64).reshape(-1), nP[:2], [u, v, s2, ur, bf]])
        af[k], ai[k] = np.concatenate([[thresh], x3d]), int(just)
    return si, sf, af, ai


@functools.lru_cache(maxsize=None)
def tables_F():
    from tests import new_points_ref as NP
    O = _oracle()
    cd, cams, _ = _cam_dicts()
    tri, nul = tri_case_lists()
    T = {}
    for M in NULL_M:
        names, ref, orc, sv, unique, As = [], [], [], [], [], []
        for name, A, ok in nul[M]:
            x, s = AR.null_vector4_ex([AR.V(r) for r in A])
            o = O.null_vector4(A) if M <= 8 else NP.null_vector4_py(A)
            names.append(name), ref.append(x), orc.append(_align(o, x)), sv.append(s), unique.append(ok), As.append(A)
        T["null%d" % M] = Table("null_vector4<%d>" % M, names, ref, orc)
        T["null%d.sv" % M], T["null%d.unique" % M], T["null%d.A" % M] = sv, unique, As
    for N in TRI_N:
        names, ref, why, margin, orc = [], [], [], [], []
        for name, slots, thresh, just, x3d in tri[N]:
            on = [s for s in slots if s[0]]
            obs = [{"cam": cd[ci], "T": AR.V(np.asarray(Tm).reshape(-1)), "n": AR.V(nP), "u": mpf(float(u)), "v": mpf(float(v)),
                    "sigma2": mpf(float(s2)), "uright": mpf(float(ur)), "bf": mpf(float(bf))} for _, ci, Tm, nP, u, v, s2, ur, bf in on]
            info = {}
            X = AR.triangulate_aw(obs, mpf(float(np.float32(thresh))), just, AR.V(x3d), info)
            oo = [(cams[ci], np.asarray(Tm, np.float64), np.asarray(nP, np.float64), np.array([u, v], np.float32), s2, ur, bf)
                  for _, ci, Tm, nP, u, v, s2, ur, bf in on]
            oX, _ = NP.triangulate_matches(O, oo, thresh, x3d, just, NP._Margins())
            names.append(name), ref.append(X), why.append(info["why"]), margin.append(float(info["margin"])), orc.append(oX)
        T["tri%d" % N] = {"names": names, "ref": ref, "why": why, "margin": margin, "oracle": orc}
    return T


def _null_ceiling(sv):
    """a singular vector moves by the perturbation over the gap to the next singular value: 64 u s_max / (s_3 - s_4)"""
    s4, s3, s1 = (float(t) for t in sv)
    return 64 * U * s1 / (s3 - s4) if s3 > s4 else None


def _tri_check(t, got_ok, got_X, who):
    """booleans equal the reference's unless a gate or a float rounding lies within 1e-12 of its boundary; the point,
    where both give one, against as written.  Returns (failures, excused, E per case or None)"""
    bad, excused, E = [], 0, []
    for k, name in enumerate(t["names"]):
        want = t["ref"][k] is not None
        if bool(got_ok[k]) != want:
            E.append(None)
            if t["margin"][k] <= EXCUSE_MARGIN:
                excused += 1
            else:
                bad.append("triangulate/%s: %s returns %s, as written %s (%s, margin %.3g)" % (
                    name, who, bool(got_ok[k]), want, t["why"][k], t["margin"][k]))
        else:
            E.append(rel_err(got_X[k], t["ref"][k]) if want else None)
    return bad, excused, E


def test_triangulation_reference_against_oracle():
    """null_vector4: the oracle's one-sided Jacobi against the singular vector by mpmath.svd_r, sign aligned; ceiling
    64 u s_max / (s_3 - s_4).  Where the null vector is not unique the residual |A x| <= 64 u s_max is asked instead.
    triangulate_matches_world: the FP64 restatement tests/new_points_ref.py returns what as written returns (empty or
    not; excused only within 1e-12 of a gate, at most 2 per 1000) and its point is within the DLT's conditioning,
    64 u s_max / (s_3 - s_4) of the homogeneous vector, scaled by |x4| / |x4[3]| to the point."""
    T, bad = tables_F(), []
    for M in NULL_M:
        t = T["null%d" % M]
        uniq, sv = T["null%d.unique" % M], T["null%d.sv" % M]
        bad += ceiling_check(t, lambda k: _null_ceiling(sv[k]) if uniq[k] else None)
        for k, name in enumerate(t.names):
            if not uniq[k]:
                r = float(_residual(T["null%d.A" % M][k], t.orc[k]) / max(sv[k][2], mpf(1)))
                if not r <= 64 * U:
                    bad.append("null_vector4<%d>/%s: |A x| / s_max = %.3g" % (M, name, r))
    for N in TRI_N:
        t = T["tri%d" % N]
        ok = [x is not None for x in t["oracle"]]
        Xs = [x if x is not None else np.zeros(3) for x in t["oracle"]]
        b, exc, E = _tri_check(t, ok, Xs, "oracle")
        bad += b
        assert exc <= EXCUSE_CAP * len(ok), exc
        e = [x for x in E if x is not None]
        print("triangulate<%d>         E_oracle worst %.3g, median %.3g over %d points; %d of %d returns excused" % (
            N, max(e), float(np.median(e)), len(e), exc, len(ok)))
        t["e_oracle"] = E
    assert not bad, "\n".join(bad)


def test_triangulation_as_written_against_exact():
    """The DLT is the reference's choice of estimator ('not the best method', camera_base.h:587), so the point is not
    compared with the scene's; what is exact is that x4 is a null vector of A to 50 digits when the rays meet, and the
    singular vector otherwise: A^T A x = s_4^2 x to 1e-40."""
    T = tables_F()
    worst = 0.0
    for M in NULL_M:
        for k, (name, A, ok) in enumerate(tri_case_lists()[1][M]):
            x, s4 = T["null%d" % M].ref[k], T["null%d.sv" % M][k][0]
            Am = AR.mpmath.matrix([AR.V(r) for r in A])
            xv = AR.mpmath.matrix(x)
            d = Am.T * (Am * xv) - s4 * s4 * xv
            g = float(max(abs(t) for t in d) / max(T["null%d.sv" % M][k][2] ** 2, mpf(1)))
            worst = max(worst, g)
            assert g <= 1e-40, (M, name, g)
    print("null_vector4           A^T A x = s4^2 x, worst gap %.3g" % worst)


def test_triangulation_cases_enter_every_branch():
    T = tables_F()
    tri, nul = tri_case_lists()
    for N in TRI_N:
        t = T["tri%d" % N]
        why = dict(zip(t["names"], t["why"]))
        assert {"ok", "parallax", "x4", "depth", "chi2"} <= set(t["why"]), set(t["why"])
        assert why["parallax-too-small"] == "parallax" and why["parallax-enough"] == "ok"
        assert why["point-behind-one-camera"] == "depth" and why["point-at-infinity/x4[3]=0"] == "x4"
        assert why["just_check_p3d/the-point"] == "ok" and why["just_check_p3d/a-wrong-point"] == "chi2"
        assert why["stereo-slots"] == "ok" and why["stereo-slot-right-image-off"] == "chi2"
        counts = {sum(1 for s in c[1] if s[0]) for c in tri[N]}
        assert counts >= set(range(2, N + 1))
        assert any(c[3] for c in tri[N]) and any(float(s[7]) != -1 for c in tri[N] for s in c[1] if s[0])
        assert {c[2] < 1 for c in tri[N]} == {True, False}
    pat = {c[0]: [int(s[0]) for s in c[1]] for c in tri[8]}
    assert pat["empty-slots-at-the-front"][0] == 0 and pat["empty-slots-at-the-end"][-1] == 0
    assert pat["empty-slots-at-the-middle"][0] == 1 and pat["empty-slots-at-the-middle"][-1] == 1 and 0 in pat["empty-slots-at-the-middle"]
    two = [c for c in tri[8] if c[0] == "two-identical-rays-and-a-third"][0][1]
    assert np.array_equal(two[0][2], two[1][2]) and two[0][4] == two[1][4]
    for M in NULL_M:
        A = {c[0]: c[1] for c in nul[M]}
        D = A["orthogonal-columns/g=0-everywhere"]
        assert all(float(D[:, p] @ D[:, q]) == 0 for p in range(4) for q in range(p + 1, 4))       # every g == 0
        assert not A["zero-column"][:, 3].any()
        assert not all(c[2] for c in nul[M]) and any((c[1] == 0).all(1).any() for c in nul[M])    # rank deficient; zero rows


@pytest.mark.gpu
def test_triangulation_on_the_device():
    out, T, bad = device_outputs(), tables_F(), []
    test_triangulation_reference_against_oracle()          # fills E_oracle of the points
    for M in NULL_M:
        t = T["null%d" % M]
        dev = out["F.null_vector4<%d>" % M].reshape(len(t.names), 4)
        uniq, sv = T["null%d.unique" % M], T["null%d.sv" % M]
        al = np.array([_align(dev[k], t.ref[k]) for k in range(len(t.names))])
        bad += t.check_device(al, skip=[n for n, u in zip(t.names, uniq) if not u])
        n2 = np.abs((dev * dev).sum(1) - 1).max()
        if not n2 / 2 <= 16 * EPS:
            bad.append("null_vector4<%d>: not a unit vector by %.3g" % (M, n2 / 2))
        for k, name in enumerate(t.names):
            if not uniq[k]:
                r = float(_residual(T["null%d.A" % M][k], dev[k]) / max(sv[k][2], mpf(1)))
                if not r <= 64 * U:
                    bad.append("null_vector4<%d>/%s: |A x| / s_max = %.3g" % (M, name, r))
    tri = tri_case_lists()[0]
    n_exc = n_ret = 0
    for N in TRI_N:
        t = T["tri%d" % N]
        dev = out["F.triangulate<%d>" % N].reshape(len(t["names"]), 4)
        b, exc, E = _tri_check(t, dev[:, 0] != 0, dev[:, 1:], "device")
        bad += b
        n_exc, n_ret = n_exc + exc, n_ret + len(E)
        worst = 0.0
        for k, name in enumerate(t["names"]):
            if tri[N][k][3]:          # just_check_p3d: x3d is an input and stays what it was
                if not np.array_equal(dev[k, 1:], tri[N][k][4]):
                    bad.append("triangulate<%d>/%s: just_check_p3d changed the point" % (N, name))
            elif E[k] is not None and t["e_oracle"][k] is not None:
                lim = 4 * max(t["e_oracle"][k], EPS)
                worst = max(worst, E[k] / lim)
                if not E[k] <= lim:
                    bad.append("triangulate<%d>/%s: error %.3g, bound %.3g" % (N, name, E[k], lim))
        print("triangulate<%d>         device worst ratio to its bound %.3f; %d of %d returns excused" % (N, worst, exc, len(E)))
    if n_exc > EXCUSE_CAP * n_ret:
        bad.append("triangulate: %d of %d returns excused, over 2 per 1000" % (n_exc, n_ret))
    assert not bad, "\n".join(bad[:60])


# ------------------------------------------------------------------ G. reductions
REDUCTIONS = [("G.block_sum<1>", 1, 256), ("G.block_sum<2>", 2, 256), ("G.block_sum<3>", 3, 256),
              ("G.block_sum<6>", 6, 256), ("G.block_sum<27>", 27, 256), ("G.block_sum_bs<1,64>", 1, 64),
              ("G.block_sum_bs<27,64>", 27, 64), ("G.block_sum_bs<1,256>", 1, 256), ("G.block_sum_bs<27,256>", 27, 256),
              ("G.block_sum_lds<28,64>", 28, 64), ("G.block_sum_lds<28,256>", 28, 256)]


def test_reduction_pool_is_what_the_test_needs():
    pool, kinds = AC.reduction_pool()
    assert pool.shape == (2, AC.POOL_BLOCKS, AC.POOL_T, AC.POOL_N) and np.isfinite(pool).all()
    assert (pool[1] == np.roll(pool[0], -1, axis=0)).all() and not (pool[1] == pool[0]).all()
    a = np.abs(pool[0, :6])
    assert a.min() < 1e-7 and a.max() > 1e7 and (pool[0, :6] < 0).any() and (pool[0, :6] > 0).any()
    assert not pool[0, 6].any()
    for part in range(8):
        nz = np.flatnonzero(np.abs(pool[0, 7 + part]).sum(1))
        assert len(nz) == 1 and nz[0] // 32 == part
    assert (pool[0, 15] == np.round(pool[0, 15])).all() and np.abs(pool[0, 15]).max() < 2 ** 21


@pytest.mark.gpu
def test_reductions_on_the_device():
    out, bad = device_outputs(), []
    pool, kinds = AC.reduction_pool()
    nb = AC.POOL_BLOCKS
    for name, N, BS in REDUCTIONS:
        r = out[name].reshape(2, nb, BS, N)
        # every thread of a block holds the same bits
        same = (r.view(np.int64) == r.view(np.int64)[:, :, :1, :]).all()
        if not same:
            bad.append("%s: the threads of a block disagree" % name)
        # the second call (data set 1 of block b) sees the data of block b + 1's first call: the same bits, so the
        # second call is unaffected by the first
        if not (r[1].view(np.int64) == np.roll(r[0], -1, axis=0).view(np.int64)).all():
            bad.append("%s: the second call in a row differs from a first call on the same data" % name)
        worst = 0.0
        for ds in range(2):
            for b in range(nb):
                v = pool[ds, b, :BS, :N]
                for i in range(N):
                    exact = math.fsum(v[:, i])
                    lim = (BS - 1) * U * math.fsum(np.abs(v[:, i]))
                    d = abs(float(mpf(float(r[ds, b, 0, i])) - mpf(exact)))
                    if kinds[(b + ds) % nb] in ("integers", "all-zero") and r[ds, b, 0, i] != exact:
                        bad.append("%s/%s: %r is not the exact sum %r" % (name, kinds[(b + ds) % nb], r[ds, b, 0, i], exact))
                    if lim:
                        worst = max(worst, d / lim)
                    if not d <= lim:
                        bad.append("%s/%s value %d: off by %.3g, bound %.3g" % (name, kinds[(b + ds) % nb], i, d, lim))
        print("%-26s worst |sum - exact| over its bound %.4f" % (name, worst))
    assert not bad, "\n".join(bad[:40])


# ------------------------------------------------------------------ the program itself
def test_program_cross_compiles_for_gfx950():
    """drift of the five headers against the program is caught without a GPU"""
    exe, log = built_program()
    assert exe is not None, log
    assert os.path.getsize(exe) > 0


def test_case_lists_stay_small():
    inp = program_inputs()
    for k, per in (("A.rotvec", 3), ("A.quat", 4), ("A.mat", 9), ("A.mul_a", 4), ("A.raw_quat", 4), ("B.pose", 7),
                   ("B.state", 22), ("C.project_P", 3), ("C.unproject_uv", 2), ("C.pinhole_uv", 2)):
        assert inp[k].size // per <= 4096, k
    assert all(np.isfinite(v).all() for v in inp.values() if v.dtype == np.float64)
    assert (inp["C.project_P"].reshape(-1, 3)[:, 2] != 0).all()
