"""The Sim3 algebra of the pose graph (csrc/sim3_device.h), called function by function and compared with a 50-digit
reference (tests/sim3_algebra_ref.py) on named cases (tests/sim3_algebra_cases.py).
tests/hip_unit/sim3_algebra_test.hip evaluates on the device, tests/emul/sim3_algebra_emul.cc on the host; nothing is
compared in C++.

Three statements meet here: the 50-digit reference (from the text of g2o's types/sim3.h and Eigen's conversions, every
branch as written), the float64 restatement (tests/pose_graph_ref.py with Libm(0)), whose distance from the 50-digit
value is E_ref(case), and the code under test.  The device -- and the host build of the same header, which is how a case
is debugged without a GPU -- stays within 4 x max(E_ref(case), dim x 2^-52) of the reference output's max-norm, part by
part (quaternion: dim 4; vectors and the scale: 3; the rows of an edge error: 7).  The branch each function takes is
handed out through S3_TAP, a macro that is empty in the library, and equals the reference's, unless the deciding value
lies within 1e-12 of its switch; the case lists are built so that nothing needs that excuse (test_case_lists_stay_small
and the branch tests hold the restatement to it on the CPU).

What the text does next to its switches, measured in 50 digits (test_*_as_written_against_exact; R against 1, t and
upsilon against |upsilon|_2, omega absolute):
  s3_exp  theta <  eps, |sigma| <  eps   R 1.7e-16 (theta^3 / 6)   t 4.3e-6 |upsilon|_2 (C = 1: |sigma| / 2 short)
          theta <  eps, |sigma| >= eps   R 1.7e-16                 t 4.4e-16
          theta >= eps, |sigma| <  eps   R 1e-46                   t 4.3e-6 |upsilon|_2
          theta >= eps, |sigma| >= eps   R 1e-46                   t 6e-46
  s3_log  d >  1 - eps, |sigma| <  eps   omega 1.4e-8 (theta^3 / 6 at theta = 4.4e-3)   upsilon 4.3e-6 |upsilon|_2
          d >  1 - eps, |sigma| >= eps   omega 1.4e-8                                   upsilon 3.1e-9
          d <= 1 - eps, |sigma| <  eps   omega 2e-43                                    upsilon 4.5e-6
          d <= 1 - eps, |sigma| >= eps   omega 5e-43                                    upsilon 3e-43
  sigma = 1e-5 exactly: exp takes the general branch, s = exp(1e-5) comes back as log s = 1e-5 - 8e-22 < eps and log takes
  C = 1 (test_log_cases_enter_every_branch pins the pair); log(exp(u)) is then 5e-6 |upsilon| off, as the text has it.
  d cannot pass 1: toRotationMatrix's diagonal is 1 - 2 (y^2 + z^2) whatever w is, so an identity of norm 1 + 1e-12
  gives d = 1 exactly.  The `d > 1` case of a drifting product is therefore the d = 1 case.

log next to pi is a property family: s3_log(s3_exp(u)) is NaN where the rounded quaternion gives d < -1 (acos), and
finite but ill-conditioned (theta / (2 sqrt(1 - d^2))) next to it.  This is the reference's text; the tests pin that
the device, the host build and the restatement agree on finite versus NaN and that a finite device result keeps the
rule:
  13 of 32 cases are NaN on the device, on the host build and in the restatement alike (all six at pi - 1e-9, four of
  six at pi, three of eight rounded unit quaternions with w = 0); E_ref of the finite ones: 3e-11 (about z) and 1.8e-6
  (generic axes) at pi - 1e-5, 3e-15 and 0.075 at pi - 1e-7, 0.33 at pi (generic-b); the device is bit for bit the
  restatement on every one of them (0.250 of its bound).

Measured (E_ref worst, at which case; median; worst ratio to its bound of the host build and of the device):
  s3_quat_to_mat     2.1e-16 near-half-turn/norm=1-1e-16                  4.4e-17   0.077   0.077
  s3_mat_to_quat     6.8e-17 trace=0                                      2.7e-17   0.019   0.019
  s3_quat_rot        3.9e-16 near-half-turn/norm=1+1e-08/v=1e4m           2.4e-17   0.146   0.146
  s3_mul             1.4e-16 negative-w/norm=1-1e-08 * generic/s=1000     3.2e-17   0.041   0.041
  s3_inverse         2.4e-16 near-half-turn/norm=1-1e-08/s=1/t=1e4m       3.0e-17   0.090   0.090
  s3_map             2.8e-16 near-half-turn/s=0.001/t=zero/p=1e4m         7.3e-17   0.104   0.104
  s3_exp             1.3e-11 theta=eps(1-2e-12)/generic-b/sigma=eps+1ulp  2.3e-16   0.250   0.250
  s3_log             5.1e-10 exp(theta=1e-4/generic-b/sigma=-eps-1ulp)    1.6e-16   0.250   0.250
  s3_edge_error      9.0     ring24/edge-4                                2.2e-14   0.250   0.250
  decisions          0 of 21 (mat_to_quat), 1080 (exp), 744 (log), 164 (edge_error) excused, host build and device
  0.250 is 1 / 4: the evaluator returns the restatement's bytes.  On all 1278 cases of exp, log and edge_error the device
  (hipcc, the device's libm, -ffp-contract=off) and the host build (g++, glibc) give the restatement's result bit for
  bit.  At the golden cases' first linearisation most edge errors are rounding alone (C = Sj Si^-1 of the same table,
  |e| about 1e-16), so E_ref is of order 1 there and the rule, which is relative to |e|, adapts by construction.

The lane functions of csrc/sim3_optimize_device.h (families O and OE; the restatement is tests/loop_optimize_ref.py;
E_ref worst, at which case; median; worst ratio to its bound of the host build and of the device):
  s3o_quat_normalize   1.6e-16 generic/norm=1+1e-08/x1                    3.1e-17   0.046   0.046
  s3o_state_from_sim3  5.0e-16 i=1/170deg/t=1e4m/s=0.001                  8.7e-17   0.189   0.189
  s3o_state_to_sim3    3.6e-16 near-half-turn/p=unit/s=0.001              1.2e-16   0.135   0.135
  s3o_inc_small        2.1e-16 dphi=1/generic-a/fix_scale=0               9.6e-17   0.058   0.058   0 of 60 branches excused
  s3o_huber            1.8e-16 th2=10/e2 = dsqr + 1 ulp                   0         0.067   0.067
  s3o_ldlt_solve       9.5e-15 p10/N=7/lambda=0                           1.6e-15   0.250   0.250
  s3o_edge<1> e        0                                                  0         0       0       0 of 72 image points excused
  s3o_edge<1> J        1.7e-14 kb8-0/s=0.5/depth=50                       8.4e-16   0.250   0.250
  s3o_edge<2> e        0                                                  0         0       0       0 of 72 image points excused
  s3o_edge<2> J        1.4e-13 kb8-0/s=2/border-left (s = 1 apart)        8.1e-15   0.250   0.250
  s3o_add_edge, chi2   2.7e-16 mode=2/pinhole-body/s=2/border-left        1.2e-16   0.044   0.044   0 of 144 Huber sides excused
  e is the same double in the reference, the restatement, the host build and the device on all 144 cases (the image point
  is a float and no case lies within 1e-12 of a float boundary), and e of the call with J == nullptr is the same bytes.
  s3o_ldlt_solve runs on the accumulators of eight golden cases' first linearisation (lambda = 0, 1e-5 x max diagonal,
  1e3; N = 6 and 7), on the optical-axis system (every point on the axis of a pinhole at the identity: the columns of p_z
  and phi_z are exactly zero, lambda = 0 must fail and does), on a negated golden system and on synthetic extras; it
  returns false on all 20 systems that must fail and leaves x alone; the 6 x 6 solve never touches x[6] nor reads row 6
  of the accumulator (filled with 1e300).
  MODE 2's ds entry is Jproj (Rcw X + tcw) (-scale^2).  At s = 1 that is Jproj Pc, which vanishes for a projection: the
  entry is rounding alone in every evaluator (E_ref 1e34 and more against a 50-digit residue of 1e-49), so there it is
  held to the bound of the cancelled sum, 4 x 7 x 2^-52 x the sum of |products| (about 1e-13 absolute), and each block
  is held to its own E_ref, so that this entry does not widen the bound of the other blocks.  On the device the KB8
  case s=1/border-top came out at 1.75 of a bound taken relative to that residue (noise against noise), which is what
  showed that the relative check says nothing there; against the summation bound it stands at 0.017.
  The Jacobian as written against 50-digit central differences through the retraction, relative to the block: MODE 1
  5e-18 in every block for the pinhole and KB8 (the quaternion's own rounding), 0.3 to 0.6 for Radtan (its d(u, v) / dP
  leaves out the radial terms of k[0], k[1]); MODE 2 dPhi 6e-18 (pinhole, KB8), dP 1.0 (not the derivative of this
  retraction), ds 9e2 to 2.5e3 absolute against a true derivative of 0 (the error does not depend on s there).

Deliberate faults, each tried on a scratch copy and not kept: the sign of B in s3_exp's theta < eps, |sigma| >= eps branch
fails test_exp_on_the_host_build (and nothing else of this file: B stands next to Omega^2, 1e-10 at most there);
`(-scale * scale)` -> `(scale * scale)` in MODE 2's scale column fails test_edges_on_the_host_build (the 48 cases with
s = 0.5 and s = 2) and nothing else of this file.

Argued and not measured: the ceilings of the reference_against_restatement tests (their docstrings) and the limits of
the as_written_against_exact tests (|sigma| / 2 from the integral form of W, |W^-1| <= pi / 2), and the summation bound
of MODE 2's ds entry at s = 1.
"""
import atexit
import ctypes
import functools
import math
import os
import shutil
import subprocess
import tempfile

import mpmath
import numpy as np
import pytest
from mpmath import mpf

from tests import loop_optimize_ref as LO
from tests import pose_graph_ref as PR
from tests import sim3_algebra_cases as SC
from tests import sim3_algebra_ref as SR
from tests.test_device_algebra import EPS, EXCUSE_CAP, EXCUSE_MARGIN, U, hipcc_flags, read_blob, rel_err, write_blob

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TAP_SLOTS = 12
LM = PR.Libm(0)
SWITCH = 0.00001

Q, V3, SC1 = (0, 4, 4), (4, 7, 3), (7, 8, 3)          # (from, to, dim) of a Sim3's parts
SIM3_PARTS = [Q, V3, SC1]
TWIST_PARTS = [(0, 3, 3), (3, 6, 3), (6, 7, 3)]
EDGE_PARTS = [(0, 7, 7)]                             # an edge error is one row of seven


def _t(a):
    return ([float(v) for v in a[0:4]], [float(v) for v in a[4:7]], float(a[7]))


def _f(S):
    return np.array(list(S[0]) + list(S[1]) + [S[2]])


class Table:
    """one function on one case list: names, the 50-digit outputs (lists of mpf, None where the text leaves the reals),
    the restatement's outputs, E_ref per case, the parts (from, to, dim) of an output, the reference's decisions"""

    def __init__(self, fn, names, ref, rst, parts, taps=None, per_part=False):
        self.fn, self.names, self.ref, self.rst, self.parts, self.taps = fn, names, ref, [np.asarray(r, np.float64) for r in rst], parts, taps
        self.e_ref = [self.err(o, r) if r is not None else math.nan for o, r in zip(self.rst, ref)]
        # per_part: every part against its own E_ref (a block that cancels to nothing must not widen the others' bound)
        self.e_part = [[rel_err(o[a:b], r[a:b]) for a, b, _ in parts] for o, r in zip(self.rst, ref)] if per_part else None
        self.floor = {}         # (case, part) -> a floor in place of dim x 2^-52, where the part's reference cancels to nothing

    def err(self, x, ref):
        return max(rel_err(x[a:b], ref[a:b]) for a, b, _ in self.parts)

    def ratio(self, x, k):
        """the worst part's error over its bound 4 x max(E_ref(case), dim x 2^-52)"""
        e = self.e_part[k] if self.e_part else [self.e_ref[k]] * len(self.parts)
        return max(rel_err(x[a:b], self.ref[k][a:b]) / (4 * max(e[i], self.floor.get((k, i), dim * EPS))) for i, (a, b, dim) in enumerate(self.parts))

    def check(self, got, who, skip=()):
        got = np.asarray(got, np.float64).reshape(len(self.names), -1)
        worst, at, bad = 0.0, "", []
        for k, name in enumerate(self.names):
            if k in skip or self.ref[k] is None:
                continue
            r = self.ratio(got[k], k)
            if not r <= worst:
                worst, at = r, name
            if not r <= 1.0:
                bad.append("%s/%s: %s error %.3g, %.3g of its bound (E_ref %.3g)" % (self.fn, name, who, self.err(got[k], self.ref[k]), r,
                                                                                       self.e_ref[k]))
        print("%-18s %s worst ratio to its bound %.3f (%s) over %d cases" % (self.fn, who, worst, at, len(self.names)))
        return bad

    def figures(self):
        e = np.array(self.e_ref)
        k = int(np.nanargmax(e))
        return "%-18s E_ref worst %.3g (%s), median %.3g" % (self.fn, e[k], self.names[k], float(np.nanmedian(e)))


def ceiling_check(t, ceil):
    bad = []
    for k, name in enumerate(t.names):
        c = ceil(k) if callable(ceil) else ceil
        if t.ref[k] is not None and c is not None and not t.e_ref[k] <= c:
            bad.append("%s/%s: restatement against 50 digits %.3g, ceiling %.3g" % (t.fn, name, t.e_ref[k], c))
    print(t.figures())
    return bad


def decisions(pairs, who):
    """[(name, got, want, margin)]: decisions equal unless the deciding value lies within EXCUSE_MARGIN of its switch
    (margin: its relative distance); -> (failures, excused)"""
    bad, excused = [], 0
    for name, got, want, margin in pairs:
        if got == want:
            continue
        if margin <= EXCUSE_MARGIN:
            excused += 1
        else:
            bad.append("%s: %s decided %s, the reference %s (%.3g from the switch)" % (name, who, got, want, margin))
    return bad, excused


# ------------------------------------------------------------------ the reference's tables
@functools.lru_cache(maxsize=None)
def tables_G():
    qs, ms, rs, ss, ps, mp_ = SC.quat_cases(), SC.mat_cases(), SC.rot_cases(), SC.sim3_cases(), SC.pair_cases(), SC.map_cases()
    T = {}
    T["s3_quat_to_mat"] = Table("s3_quat_to_mat", [c[0] for c in qs], [SR.quat_to_mat(SR.V(c[1])) for c in qs],
                                [PR.quat_to_mat([float(v) for v in c[1]]) for c in qs], [(0, 9, 3)])
    T["s3_mat_to_quat"] = Table("s3_mat_to_quat", [c[0] for c in ms], [SR.mat_to_quat(SR.V(c[1])) for c in ms],
                                [PR.mat_to_quat([float(v) for v in c[1]], LM) for c in ms], [(0, 4, 4)],
                                taps=[SR.mat_to_quat_branch(SR.V(c[1])) for c in ms])
    T["s3_quat_rot"] = Table("s3_quat_rot", [c[0] for c in rs], [SR.quat_rot(SR.V(c[1]), SR.V(c[2])) for c in rs],
                             [PR.quat_rot([float(v) for v in c[1]], [float(v) for v in c[2]]) for c in rs], [(0, 3, 3)])
    T["s3_mul"] = Table("s3_mul", [c[0] for c in ps], [SR.mul(SR.V(c[1]), SR.V(c[2])) for c in ps],
                        [_f(PR.mul(_t(c[1]), _t(c[2]))) for c in ps], SIM3_PARTS)
    T["s3_inverse"] = Table("s3_inverse", [c[0] for c in ss], [SR.inverse(SR.V(c[1])) for c in ss],
                            [_f(PR.inverse(_t(c[1]))) for c in ss], SIM3_PARTS)
    T["s3_map"] = Table("s3_map", [c[0] for c in mp_], [SR.smap(SR.V(c[1]), SR.V(c[2])) for c in mp_],
                        [PR.smap(_t(c[1]), [float(v) for v in c[2]]) for c in mp_], [(0, 3, 3)])
    return T


@functools.lru_cache(maxsize=None)
def table_X():
    cs = SC.exp_cases()
    out = [SR.exp(SR.V(c[1])) for c in cs]
    return Table("s3_exp", [c[0] for c in cs], [o[0] for o in out], [_f(PR.exp([float(v) for v in c[1]], LM)) for c in cs], SIM3_PARTS,
                 taps=[o[1] for o in out])


def _log_table(fn, cs):
    out = [SR.log(SR.V(c[1])) for c in cs]
    with np.errstate(all="ignore"):
        rst = []
        for c in cs:
            try:
                rst.append(PR.log(_t(c[1]), LM))
            except (ValueError, ZeroDivisionError):      # math.acos outside [-1, 1], 1 - d^2 = 0: NaN in C
                rst.append([math.nan] * 7)
    return Table(fn, [c[0] for c in cs], [o[0] for o in out], rst, TWIST_PARTS, taps=[o[1] for o in out])


@functools.lru_cache(maxsize=None)
def table_L():
    return _log_table("s3_log", SC.log_cases())


@functools.lru_cache(maxsize=None)
def table_P():
    return _log_table("s3_log near pi", SC.log_near_pi_cases())


@functools.lru_cache(maxsize=None)
def table_E():
    cs = SC.edge_cases()
    out = [SR.edge_error(SR.V(c[1]), SR.V(c[2]), SR.V(c[3])) for c in cs]
    return Table("s3_edge_error", [c[0] for c in cs], [o[0] for o in out], [PR.edge_error(_t(c[1]), _t(c[2]), _t(c[3]), LM) for c in cs],
                 EDGE_PARTS, taps=[o[1] for o in out])


# ------------------------------------------------------------------ the program, its inputs, the two evaluators
def _stack(cases, k):
    return np.array([c[k] for c in cases], np.float64)


@functools.lru_cache(maxsize=None)
def program_inputs():
    return {"G.quat": _stack(SC.quat_cases(), 1), "G.mat": _stack(SC.mat_cases(), 1), "G.rot_q": _stack(SC.rot_cases(), 1),
            "G.rot_v": _stack(SC.rot_cases(), 2), "G.mul_a": _stack(SC.pair_cases(), 1), "G.mul_b": _stack(SC.pair_cases(), 2),
            "G.sim3": _stack(SC.sim3_cases(), 1), "G.map_S": _stack(SC.map_cases(), 1), "G.map_p": _stack(SC.map_cases(), 2),
            "X.u": _stack(SC.exp_cases(), 1), "L.S": _stack(SC.log_cases(), 1), "P.S": _stack(SC.log_near_pi_cases(), 1),
            "E.C": _stack(SC.edge_cases(), 1), "E.Si": _stack(SC.edge_cases(), 2), "E.Sj": _stack(SC.edge_cases(), 3),
            "O.raw_quat": _stack(SC.raw_quat_cases(), 1), "O.Rts": _stack(SC.from_sim3_cases(), 1), "O.state": _stack(SC.state_cases(), 1),
            "O.inc_state": _stack(SC.inc_small_cases(), 1), "O.inc_d": _stack(SC.inc_small_cases(), 2),
            "O.huber": _stack(SC.huber_cases(), 1), "O.ldlt": _stack(SC.ldlt_cases(), 1),
            "O.edge": _stack(SC.s3o_edge_cases(), 1), "O.cams": SC.edge_cam_table(), "O.add_edge": _stack(SC.add_edge_cases(), 1)}


@functools.lru_cache(maxsize=None)
def built_program():
    flags, hipcc = hipcc_flags()
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc") or hipcc
    d = tempfile.mkdtemp(prefix="sim3_algebra_")
    atexit.register(shutil.rmtree, d, True)
    exe = os.path.join(d, "sim3_algebra_test")
    r = subprocess.run([hipcc] + flags + ["-o", exe, os.path.join(HERE, "hip_unit", "sim3_algebra_test.hip")], capture_output=True, text=True)
    if r.returncode != 0:
        return None, r.stdout + r.stderr
    return exe, r.stdout + r.stderr


@functools.lru_cache(maxsize=None)
def device_run():
    """("ok", outputs) or ("failed", message): built once, fed once, run once; a failure is cached and every test reports
    it without starting the program again"""
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
    out = read_blob(fout)
    for k in [k for k in out if k.endswith("tap")]:       # the tap area has a row for every lane of the launch
        out[k] = out[k].reshape(-1, TAP_SLOTS)
    return "ok", out


def device_outputs():
    st, out = device_run()
    assert st == "ok", out
    return out


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


@functools.lru_cache(maxsize=None)
def host_outputs():
    """the arrays the program writes, from the host build of the same header"""
    out_so = os.path.join(HERE, "emul", "libsim3_algebra_emul.so")
    deps = [os.path.join(HERE, "emul", "sim3_algebra_emul.cc")] + [os.path.join(ROOT, "vieo_slam_amd", "csrc", h) for h in (
        "sim3_device.h", "sim3_optimize_device.h", "cam_project.h", "lba_policy.h")]
    if not os.path.exists(out_so) or any(os.path.getmtime(d) > os.path.getmtime(out_so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", out_so, deps[0], "-lm"])
    L = ctypes.CDLL(out_so)
    assert L.emul_s3a_tap_slots() == TAP_SLOTS
    inp, out = program_inputs(), {}

    def run(fn, name, width, *arrays, tap=None):
        n = len(arrays[0])
        o = np.zeros((n, width))
        args = [n] + [_p(np.ascontiguousarray(a)) for a in arrays] + [_p(o)]
        if tap:
            out[tap] = np.zeros((n, TAP_SLOTS))
            args.append(_p(out[tap]))
        fn(*args)
        out[name] = o.reshape(-1)
    run(L.emul_s3a_quat_to_mat, "G.s3_quat_to_mat", 9, inp["G.quat"])
    run(L.emul_s3a_mat_to_quat, "G.s3_mat_to_quat", 4, inp["G.mat"], tap="G.mat_to_quat.tap")
    run(L.emul_s3a_quat_rot, "G.s3_quat_rot", 3, inp["G.rot_q"], inp["G.rot_v"])
    run(L.emul_s3a_mul, "G.s3_mul", 8, inp["G.mul_a"], inp["G.mul_b"])
    run(L.emul_s3a_inverse, "G.s3_inverse", 8, inp["G.sim3"])
    run(L.emul_s3a_map, "G.s3_map", 3, inp["G.map_S"], inp["G.map_p"])
    run(L.emul_s3a_exp, "X.s3_exp", 8, inp["X.u"], tap="X.tap")
    run(L.emul_s3a_log, "L.s3_log", 7, inp["L.S"], tap="L.tap")
    run(L.emul_s3a_log, "P.s3_log", 7, inp["P.S"], tap="P.tap")
    run(L.emul_s3a_edge_error, "E.s3_edge_error", 7, inp["E.C"], inp["E.Si"], inp["E.Sj"], tap="E.tap")
    run(L.emul_s3a_quat_normalize, "O.s3o_quat_normalize", 4, inp["O.raw_quat"])
    run(L.emul_s3a_state_from_sim3, "O.s3o_state_from_sim3", 8, inp["O.Rts"])
    run(L.emul_s3a_state_to_sim3, "O.s3o_state_to_sim3", 13, inp["O.state"])
    run(L.emul_s3a_inc_small, "O.s3o_inc_small", 8, inp["O.inc_state"], inp["O.inc_d"], tap="O.inc_small.tap")
    run(L.emul_s3a_edge, "O.s3o_edge", 18, inp["O.edge"], inp["O.cams"])
    run(L.emul_s3a_add_edge, "O.s3o_add_edge", 37, inp["O.add_edge"])
    run(L.emul_s3a_huber, "O.s3o_huber", 2, inp["O.huber"])
    run(L.emul_s3a_ldlt, "O.s3o_ldlt_solve", 8, inp["O.ldlt"])
    return out


# ------------------------------------------------------------------ decisions: the reference's, the restatement's, the taps
def _rel(x, at):
    return float(abs(x - at) / abs(at)) if at != 0 else float(abs(x))


def m2q_pairs(names, mats, got, taps):
    """got: branch numbers (0: trace > 0, 1 + i).  The margin of a case is how close the trace is to 0 or, beyond it, the
    two diagonal entries that decide are to each other."""
    out = []
    for k, name in enumerate(names):
        br, tr = taps[k]
        R = SR.V(mats[k])
        m = float(abs(tr))
        if br != 0 and got[k] != 0:
            m = float(min(abs(R[4] - R[0]), abs(R[8] - R[4]), abs(R[8] - R[0])))
        out.append(("s3_mat_to_quat/" + name, int(got[k]), br, m))
    return out


def exp_pairs(names, us, small_theta, sigma_small, taps):
    out = []
    for k, name in enumerate(names):
        out.append(("s3_exp theta/" + name, bool(small_theta[k]), bool(taps[k]["small_theta"]), _rel(taps[k]["theta"], SR.EPS)))
        out.append(("s3_exp sigma/" + name, bool(sigma_small[k]), bool(taps[k]["sigma_small"]), _rel(abs(mpf(float(us[k][6]))), SR.EPS)))
    return out


def log_pairs(fn, names, near, sigma_small, taps):
    out = []
    for k, name in enumerate(names):
        out.append(("%s d/%s" % (fn, name), bool(near[k]), bool(taps[k]["near_identity"]), _rel(taps[k]["d"], 1 - SR.EPS)))
        out.append(("%s sigma/%s" % (fn, name), bool(sigma_small[k]), bool(taps[k]["sigma_small"]), _rel(abs(taps[k]["sigma"]), SR.EPS)))
    return out


def rst_m2q_branch(R):
    t = R[0] + R[4] + R[8]
    if t > 0:
        return 0
    i = 0
    if R[4] > R[0]:
        i = 1
    if R[8] > R[4 * i]:
        i = 2
    return 1 + i


def rst_exp_decisions(u):
    return math.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) < SWITCH, abs(u[6]) < SWITCH


def rst_log_decisions(S):
    R = PR.quat_to_mat([float(v) for v in S[0:4]])
    return 0.5 * (R[0] + R[4] + R[8] - 1) > 1 - SWITCH, abs(math.log(float(S[7]))) < SWITCH


def rst_edge_decisions(c):
    return rst_log_decisions(_f(PR.mul(PR.mul(_t(c[1]), _t(c[2])), PR.inverse(_t(c[3])))))


def cap(excused, n, what):
    assert excused <= EXCUSE_CAP * n, "%s: %d of %d decisions excused" % (what, excused, n)
    print("%-18s %d of %d decisions excused" % (what, excused, n))


def check_taps(out, who):
    """the branch taps of an evaluator against the reference's decisions, family by family"""
    bad = []
    ms, xs, ls, es = SC.mat_cases(), SC.exp_cases(), SC.log_cases(), SC.edge_cases()
    t = out["G.mat_to_quat.tap"]
    b, x = decisions(m2q_pairs([c[0] for c in ms], [c[1] for c in ms], t[:len(ms), 0], tables_G()["s3_mat_to_quat"].taps), who)
    cap(x, len(ms), "s3_mat_to_quat")
    bad += b
    t, X = out["X.tap"], table_X()
    b, x = decisions(exp_pairs(X.names, [c[1] for c in xs], t[:len(xs), 2], t[:len(xs), 4], X.taps), who)
    b2, x2 = decisions([("s3_exp -> mat_to_quat/" + n, int(t[k, 0]), X.taps[k]["m2q"], float(abs(X.taps[k]["trace"]))) for k, n in enumerate(X.names)], who)
    cap(x + x2, 3 * len(xs), "s3_exp")
    bad += b + b2
    for key, T, n in (("L.tap", table_L(), len(ls)), ("E.tap", table_E(), len(es))):
        t = out[key]
        b, x = decisions(log_pairs(T.fn, T.names, t[:n, 5], t[:n, 7], T.taps), who)
        cap(x, 2 * n, T.fn)
        bad += b
    return bad


# ------------------------------------------------------------------ G. conversions and group operations
def test_conversions_reference_against_restatement():
    """E_ref ceilings: a handful of roundings on terms no larger than the output (the translations of the cases do not
    cancel): 32 u of the part's max-norm."""
    bad = []
    for t in tables_G().values():
        bad += ceiling_check(t, 32 * U)
    assert not bad, "\n".join(bad)


def test_conversion_cases_enter_every_branch():
    """from the inputs themselves; the restatement decides as the reference does on every case, with no excuse"""
    ms = SC.mat_cases()
    taps = tables_G()["s3_mat_to_quat"].taps
    names = [c[0] for c in ms]
    assert {0, 1, 2, 3} <= {b for b, _ in taps}
    tr = {n: float(t) for n, (_, t) in zip(names, taps)}
    assert 0 < tr["trace+1e-12"] < 2e-12 and -2e-12 < tr["trace-1e-12"] < 0 and 0 < tr["trace+1ulp"] < 1e-16 and -1e-16 < tr["trace-1ulp"] < 0
    assert tr["trace=0"] == 0 and taps[names.index("trace=0")][0] != 0 and taps[names.index("trace=0/120deg-about-111")][0] != 0
    assert taps[names.index("tie-R4=R0")][0] == 1 and taps[names.index("tie-R8=R4")][0] == 2 and taps[names.index("tie-R8=R0")][0] == 1
    assert taps[names.index("tie-all")][0] == 1
    bad, x = decisions(m2q_pairs(names, [c[1] for c in ms], [rst_m2q_branch([float(v) for v in c[1]]) for c in ms], taps), "the restatement")
    assert not bad and x == 0, "\n".join(bad)
    norms = [abs(float(np.linalg.norm(c[1])) - 1) for c in SC.quat_cases()]
    assert any(5e-9 < n < 2e-8 for n in norms) and any(5e-13 < n < 2e-12 for n in norms) and any(n < 3e-16 for n in norms)
    S = _stack(SC.sim3_cases(), 1)
    assert set(S[:, 7]) == {1e-3, 1.0, 1e3} and np.abs(S[:, 4:7]).max() == 1e4


def _check_G(out, who):
    bad = []
    for fn, t in tables_G().items():
        bad += t.check(out["G." + fn], who)
    return bad


def test_conversions_on_the_host_build():
    out = host_outputs()
    bad = _check_G(out, "host build")
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_conversions_on_the_device():
    out = device_outputs()
    bad = _check_G(out, "device")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------ X. s3_exp
def _exp_ceiling(k):
    """A, B and C cancel in their numerators: cos's and exp's rounding u over theta^2 + sigma^2, next to Omega (theta)
    and sigma: u / theta where theta >= eps, u / |sigma| where |sigma| >= eps, on top of 64 u of plain roundings"""
    u = SC.exp_cases()[k][1]
    th, sg = float(np.linalg.norm(u[:3])), abs(float(u[6]))
    return 64 * U * (1 + (1 / th if th >= SWITCH * (1 - 1e-9) else 0) + (1 / sg if sg >= SWITCH else 0))


def test_exp_reference_against_restatement():
    bad = ceiling_check(table_X(), _exp_ceiling)
    assert not bad, "\n".join(bad)


def test_exp_cases_enter_every_branch():
    X, cs = table_X(), SC.exp_cases()
    seen = {(t["small_theta"], t["sigma_small"]) for t in X.taps}
    assert seen == {(True, True), (True, False), (False, True), (False, False)}
    th = [float(t["theta"]) for t in X.taps]
    for v in (0.0, SC.BELOW, SC.SWITCH, SC.ABOVE, 1e-4, 0.5, 3.0, math.pi - 1e-3):
        assert v in th, v                                     # (exact along the coordinate axis)
    assert {float(c[1][6]) for c in cs} == set(SC.SIGMAS)
    assert any(t["m2q"] != 0 for t in X.taps) and any(t["m2q"] == 0 for t in X.taps)
    rd = [rst_exp_decisions([float(v) for v in c[1]]) for c in cs]
    bad, x = decisions(exp_pairs(X.names, [c[1] for c in cs], [d[0] for d in rd], [d[1] for d in rd], X.taps), "the restatement")
    assert not bad and x == 0, "\n".join(bad)


def test_exp_as_written_against_exact():
    """The text against the exponential of the generator, in 50 digits, per branch: R relative to 1, t relative to
    |upsilon|_2.  General branch: equal (1e-40).  theta < eps: R = I + Omega + Omega^2 / 2 drops theta^3 / 6 (1.7e-16 at
    the switch), A = 1 / 2 and B = 1 / 6 drop theta^2 / 24 and theta^2 / 120 next to factors theta and theta^2.
    |sigma| < eps: the text takes W at sigma = 0; W = int_0^1 e^(tau sigma) R(tau theta) dtau, so it is
    int (e^(tau sigma) - 1) R short, |sigma| / 2 (1 + |sigma|) in the 2-norm: t is off by up to 5.1e-6 |upsilon|, the
    1e-5 of the sigma switch."""
    worst = {}
    bad = []
    X = table_X()
    for k, (name, u) in enumerate(SC.exp_cases()):
        S, tp = X.ref[k], X.taps[k]
        sR, t, s = SR.exp_exact(SR.V(u))
        R = SR.quat_to_mat(S[0:4])
        gR = float(max(abs(S[7] * a - b) for a, b in zip(R, sR)) / s)
        nu = float(np.linalg.norm(u[3:6]))
        gt = float(max(abs(a - b) for a, b in zip(S[4:7], t))) / (nu if nu != 0 else 1)
        key = ("theta < eps" if tp["small_theta"] else "theta >= eps") + (", |sigma| < eps" if tp["sigma_small"] else ", |sigma| >= eps")
        w = worst.setdefault(key, [0.0, 0.0])
        w[0], w[1] = max(w[0], gR), max(w[1], gt)
        th, sg = float(tp["theta"]), abs(float(u[6]))
        limR = 1e-30 + (th ** 3 / 5 if tp["small_theta"] else 0)
        limt = 1e-30 + (0.51 * sg if tp["sigma_small"] else 0) + (th ** 3 if tp["small_theta"] else 0)
        if not (gR <= limR and gt <= limt):
            bad.append("s3_exp/%s: R off by %.3g (limit %.3g), t by %.3g (limit %.3g)" % (name, gR, limR, gt, limt))
    for key, (gR, gt) in sorted(worst.items()):
        print("s3_exp as written against exact, %-32s R %.3g, t %.3g" % (key, gR, gt))
    assert not bad, "\n".join(bad)


def test_exp_on_the_host_build():
    bad = table_X().check(host_outputs()["X.s3_exp"], "host build")
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_exp_on_the_device():
    bad = table_X().check(device_outputs()["X.s3_exp"], "device")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------ L. s3_log, E. s3_edge_error
def _log_ceiling(T, k, extra=1.0):
    """acos and theta / (2 sqrt(1 - d^2)) carry d's rounding u over 1 - d^2; deltaR cancels to u next to theta; A, B, C as
    in exp: 64 u (1 + 1 / theta + 1 / (1 - d^2) + 1 / |sigma|).  With d > 1 - eps and |sigma| >= eps the limits
    A = ((sigma - 1) s + 1) / sigma^2 and B = (...) / sigma^3 cancel to u / sigma^2 and u / sigma^3 next to Omega and
    Omega^2, and theta reaches 4.47e-3 there: theta / sigma^2 + theta^2 / sigma^3 more."""
    tp = T.taps[k]
    d, sg = float(tp["d"]), abs(float(tp["sigma"]))
    th = float(max(abs(v) for v in T.ref[k][0:3]))
    c = 1 + (1 / th if th > 0 else 0) + (1 / sg if sg >= SWITCH * (1 - 1e-9) else 0)
    if not tp["near_identity"]:
        c += 1 / (1 - d * d)
    elif sg >= SWITCH * (1 - 1e-9):
        c += th / sg ** 2 + th ** 2 / sg ** 3
    return 64 * U * c * extra


def test_log_reference_against_restatement():
    T = table_L()
    bad = ceiling_check(T, lambda k: _log_ceiling(T, k))
    assert not bad, "\n".join(bad)


def test_edge_error_reference_against_restatement():
    """as log, times the cancellation of the product: the unit quaternions and the largest translation among C, Si, Sj
    (scaled) over the error's max-norm.  At the golden cases' first linearisation most errors are rounding alone
    (C = Sj Si^-1 of the same table): E_ref is of order 1 there and the ceiling says nothing."""
    T, cs = table_E(), SC.edge_cases()

    def ceil(k):
        big = max(float(np.abs(c[4:7]).max()) * max(1.0, 1 / c[7]) for c in cs[k][1:4])
        small = float(max(abs(v) for v in T.ref[k]))
        return _log_ceiling(T, k, extra=1 + (1 + big) / max(small, 1e-300))
    bad = ceiling_check(T, ceil)
    assert not bad, "\n".join(bad)


def test_log_cases_enter_every_branch():
    L, cs = table_L(), SC.log_cases()
    assert all(r is not None for r in L.ref)
    seen = {(t["near_identity"], t["sigma_small"]) for t in L.taps}
    assert seen == {(True, True), (True, False), (False, True), (False, False)}
    names = L.names
    d = {n: t["d"] for n, t in zip(names, L.taps)}
    assert d["theta=4.4e-3/axis=z"] > 1 - SR.EPS > d["theta=4.5e-3/axis=z"]
    hi, lo = d["d=(1-eps)(1+2e-12)/s=1"], d["d=(1-eps)(1-2e-12)/s=1"]
    assert EXCUSE_MARGIN < _rel(hi, 1 - SR.EPS) < 3e-12 and hi > 1 - SR.EPS
    assert EXCUSE_MARGIN < _rel(lo, 1 - SR.EPS) < 3e-12 and lo < 1 - SR.EPS
    assert d["identity/norm=1+1e-12"] == 1                     # (d cannot pass 1: the diagonal does not see w)
    # sigma recomputed across eps: exp took its general branch on sigma = 1e-5, log takes C = 1
    k = names.index("exp(theta=0.5/axis=generic-a/sigma=%.17g/upsilon=generic)" % SWITCH)
    assert L.taps[k]["sigma_small"] and not table_X().taps[table_X().names.index(names[k][4:-1])]["sigma_small"]
    assert max(float(mpmath.acos(t["d"])) for t in L.taps) > math.pi - 1.1e-3
    rd = [rst_log_decisions(c[1]) for c in cs]
    bad, x = decisions(log_pairs("s3_log", names, [r[0] for r in rd], [r[1] for r in rd], L.taps), "the restatement")
    assert not bad and x == 0, "\n".join(bad)


def test_edge_error_cases_enter_every_branch():
    E, cs = table_E(), SC.edge_cases()
    assert all(r is not None for r in E.ref)
    prod = [t for n, t in zip(E.names, E.taps) if n.startswith("product/")]
    assert {(t["near_identity"], t["sigma_small"]) for t in prod} == {(True, True), (True, False), (False, True), (False, False)}
    assert sum(n.startswith("ring24/") for n in E.names) >= 24 and sum(n.startswith("scale16/") for n in E.names) >= 16
    rd = [rst_edge_decisions(c) for c in cs]
    bad, x = decisions(log_pairs("s3_edge_error", E.names, [r[0] for r in rd], [r[1] for r in rd], E.taps), "the restatement")
    assert not bad and x == 0, "\n".join(bad)


def test_log_as_written_against_exact():
    """log as written, on the exact exponential of a twist (50 digits, no rounding), against the twist.  General branch:
    equal.  d > 1 - eps: omega = 0.5 deltaR is sin(theta) / theta omega, theta^2 / 6 short (3.3e-6 relative, 1.5e-8
    absolute at the switch theta = 4.47e-3), and A = 1 / 2, B = 1 / 6 move upsilon by theta^2 / 12-class terms.
    |sigma| < eps: W is taken at sigma = 0, |sigma| / 2 short (see exp), and |W^-1| <= pi / 2 up to theta = pi: upsilon is
    off by up to 8.1e-6 |upsilon|_2.  d > 1 - eps moves upsilon by theta^3-class terms; theta^2 is asked."""
    worst, bad = {}, []
    twists = [c for c in SC.exp_cases() if "upsilon=generic" in c[0]]
    twists += [("theta=%g/%s" % (th, an), np.array([th * a for a in ax] + [0.3, -1.2, 2.0, sg])) for th in (4.4e-3, 4.5e-3)
               for an, ax in SC.AXES for sg in (0.0, 0.1)]
    for name, u in twists:
        um = SR.V(u)
        sR, t, s = SR.exp_exact(um)
        S = SR.mat_to_quat([v / s for v in sR]) + t + [s]
        res, tp = SR.log(S)
        assert res is not None, name
        th = float(mpmath.sqrt(sum(v * v for v in um[0:3])))
        g_om = float(max(abs(a - b) for a, b in zip(res[0:3], um[0:3])))
        g_up = float(max(abs(a - b) for a, b in zip(res[3:6], um[3:6]))) / float(np.linalg.norm(u[3:6]))
        key = ("d > 1 - eps" if tp["near_identity"] else "d <= 1 - eps") + (", |sigma| < eps" if tp["sigma_small"] else ", |sigma| >= eps")
        w = worst.setdefault(key, [0.0, 0.0])
        w[0], w[1] = max(w[0], g_om), max(w[1], g_up)
        lim_om = 1e-30 + (th ** 3 / 5.9 if tp["near_identity"] else 0)
        lim_up = 1e-30 + (0.81 * abs(float(u[6])) if tp["sigma_small"] else 0) + (th ** 2 if tp["near_identity"] else 0)
        if not (g_om <= lim_om and g_up <= lim_up):
            bad.append("s3_log/%s: omega off by %.3g (limit %.3g), upsilon by %.3g (limit %.3g)" % (name, g_om, lim_om, g_up, lim_up))
    for key, (a, b) in sorted(worst.items()):
        print("s3_log as written against exact, %-32s omega %.3g (absolute), upsilon %.3g" % (key, a, b))
    assert not bad, "\n".join(bad)


def test_log_and_edge_error_on_the_host_build():
    out = host_outputs()
    bad = table_L().check(out["L.s3_log"], "host build") + table_E().check(out["E.s3_edge_error"], "host build")
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_log_and_edge_error_on_the_device():
    out = device_outputs()
    bad = table_L().check(out["L.s3_log"], "device") + table_E().check(out["E.s3_edge_error"], "device")
    assert not bad, "\n".join(bad)


def test_branches_on_the_host_build():
    bad = check_taps(host_outputs(), "the host build")
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_branches_on_the_device():
    bad = check_taps(device_outputs(), "the device")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------ P. log next to pi
def _near_pi(got, who):
    """finite or NaN as the restatement; a finite result within the rule where the 50-digit reference is real"""
    P = table_P()
    got = np.asarray(got).reshape(len(P.names), 7)
    bad, n_nan = [], 0
    for k, name in enumerate(P.names):
        fin_r, fin_g = bool(np.isfinite(P.rst[k]).all()), bool(np.isfinite(got[k]).all())
        n_nan += not fin_g
        if fin_r != fin_g:
            bad.append("%s: %s is %s, the restatement %s" % (name, who, "finite" if fin_g else "not finite", "finite" if fin_r else "not finite"))
        elif fin_g and P.ref[k] is not None:
            r = P.ratio(got[k], k)
            print("s3_log near pi/%-44s E_ref %.3g, %s at %.3f of its bound" % (name, P.e_ref[k], who, r))
            if not r <= 1.0:
                bad.append("%s: %s at %.3g of its bound (E_ref %.3g)" % (name, who, r, P.e_ref[k]))
    print("s3_log near pi: %d of %d results of %s are not finite" % (n_nan, len(P.names), who))
    return bad


def test_log_near_pi_on_the_host_build():
    P = table_P()
    assert any(not np.isfinite(r).all() for r in P.rst) and any(np.isfinite(r).all() for r in P.rst)
    bad = _near_pi(host_outputs()["P.s3_log"], "the host build")
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_log_near_pi_on_the_device():
    bad = _near_pi(device_outputs()["P.s3_log"], "the device")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------ O. OptimizeSim3's state functions, Huber, the small LDL^T
STATE_PARTS = [(0, 3, 3), (3, 7, 4), (7, 8, 3)]


def _st(a):
    return ([float(v) for v in a[0:3]], [float(v) for v in a[3:7]], float(a[7]))


def _fst(st):
    return np.array(list(st[0]) + list(st[1]) + [st[2]])


@functools.lru_cache(maxsize=None)
def tables_O():
    rq, fs, sc, ic, hc, lc = SC.raw_quat_cases(), SC.from_sim3_cases(), SC.state_cases(), SC.inc_small_cases(), SC.huber_cases(), SC.ldlt_cases()
    T = {}
    T["s3o_quat_normalize"] = Table("s3o_quat_normalize", [c[0] for c in rq], [SR.quat_normalize(SR.V(c[1])) for c in rq],
                                    [LO._qnormalize([float(v) for v in c[1]], LM) for c in rq], [(0, 4, 4)])
    T["s3o_state_from_sim3"] = Table("s3o_state_from_sim3", [c[0] for c in fs],
                                     [SR.state_from_sim3(SR.V(c[1][0:9]), SR.V(c[1][9:12]), mpf(float(c[1][12]))) for c in fs],
                                     [_fst(LO.state_from_sim3(c[1][0:9], c[1][9:12], c[1][12], LM)) for c in fs], STATE_PARTS)
    to = []
    for c in sc:
        s12, R12, t12 = LO.state_to_sim3(_st(c[1]), LM)
        to.append(np.concatenate([R12.reshape(-1), t12, [s12]]))
    T["s3o_state_to_sim3"] = Table("s3o_state_to_sim3", [c[0] for c in sc], [SR.state_to_sim3(SR.V(c[1])) for c in sc], to,
                                   [(0, 9, 3), (9, 12, 3), (12, 13, 3)])
    inc = [SR.inc_small(SR.V(c[1]), SR.V(c[2][0:7]), c[2][7] != 0) for c in ic]
    T["s3o_inc_small"] = Table("s3o_inc_small", [c[0] for c in ic], [o[0] for o in inc],
                               [_fst(LO.inc_small(_st(c[1]), [float(v) for v in c[2][0:7]], c[2][7] != 0, LM)) for c in ic], STATE_PARTS,
                               taps=[o[1] for o in inc])
    hub = [SR.huber(*SR.V(c[1])) for c in hc]
    rst = [[float(v[0]) for v in LO.huber(np.array([c[1][0]]), c[1][1], c[1][2], LM)] for c in hc]
    T["s3o_huber"] = Table("s3o_huber", [c[0] for c in hc], [o[0] for o in hub], rst, [(0, 1, 3), (1, 2, 3)], taps=[o[1] for o in hub])
    ref, rst, names = [], [], []
    for c in lc:
        n = int(c[1][37])
        x, _ = SR.ldlt_solve(SR.V(c[1][0:36]), mpf(float(c[1][36])), n)
        r = LO.ldlt_solve(c[1][0:36], float(c[1][36]), n)
        assert (x is None) == (r is None) == c[2], c[0]         # the restatement decides as the reference, no excuse
        names.append(c[0]), ref.append(x), rst.append(np.zeros(7) if r is None else np.array(r))
    T["s3o_ldlt_solve"] = Table("s3o_ldlt_solve", names, ref, rst, [(0, 7, 7)])
    return T


def test_state_functions_reference_against_restatement():
    """E_ref ceilings.  Normalisations, products and rotations of O(1) terms: 32 u.  s3o_ldlt_solve: 64 u times the
    condition number of the leading block of H + lambda I (numpy's, from the case's own accumulators)."""
    T, bad = tables_O(), []
    for fn in ("s3o_quat_normalize", "s3o_state_from_sim3", "s3o_state_to_sim3", "s3o_inc_small", "s3o_huber"):
        bad += ceiling_check(T[fn], 32 * U)
    lc = SC.ldlt_cases()

    def cond(k):
        a, n = lc[k][1], int(lc[k][1][37])
        H = np.zeros((7, 7))
        H[np.triu_indices(7)] = a[0:28]
        H = (H + np.triu(H, 1).T)[:n, :n] + a[36] * np.eye(n)
        return 64 * U * float(np.linalg.cond(H))
    bad += ceiling_check(T["s3o_ldlt_solve"], cond)
    assert not bad, "\n".join(bad)


def test_state_function_cases_enter_every_branch():
    T = tables_O()
    th = [float(np.linalg.norm(c[2][3:6])) for c in SC.inc_small_cases()]
    for v in SC.DPHIS:
        assert v in th, v                                       # 0, the switch and one ulp either side, 1, 3: exact along z
    assert {bool(t) for t in T["s3o_inc_small"].taps} == {True, False}
    assert {c[2][7] for c in SC.inc_small_cases()} == {0.0, 1.0}
    hub = {n.split("/")[1]: t for n, t in zip(T["s3o_huber"].names, T["s3o_huber"].taps) if n.startswith("th2=10/")}
    assert hub["e2=dsqr"] and hub["e2dsqr-1ulp"] and not hub["e2dsqr+1ulp"] and hub["e20"] and not hub["e21e12"]
    lc = SC.ldlt_cases()
    assert sum(c[2] for c in lc) == 20 and sum(c[0].startswith("optical-axis") and c[2] for c in lc) == 2 and {int(c[1][37]) for c in lc} == {6, 7}
    assert all(c[1][6] == 1e300 and c[1][34] == 1e300 for c in lc if int(c[1][37]) == 6 and not c[2])     # the guard of N = 6
    br = {SR.mat_to_quat_branch(SR.V(c[1][0:9]))[0] for c in SC.from_sim3_cases()}
    assert br == {0, 1, 2, 3}


def _check_O(out, who):
    T, bad = tables_O(), []
    for fn in ("s3o_quat_normalize", "s3o_state_from_sim3", "s3o_state_to_sim3", "s3o_inc_small", "s3o_huber"):
        bad += T[fn].check(out["O." + fn], who)
    ic, tap = SC.inc_small_cases(), out["O.inc_small.tap"]
    b, x = decisions([("s3o_inc_small theta/" + c[0], bool(tap[k, 9]), bool(T["s3o_inc_small"].taps[k]),
                       _rel(mpmath.sqrt(sum(mpf(float(v)) ** 2 for v in c[2][3:6])), SR.EPS)) for k, c in enumerate(ic)], who)
    cap(x, len(ic), "s3o_inc_small")
    bad += b
    # Huber's side: rho' = 1 exactly on the inlier side; one ulp from dsqr either side may go
    hub, hc = np.asarray(out["O.s3o_huber"]).reshape(-1, 2), SC.huber_cases()
    b, x = decisions([("s3o_huber/" + c[0], bool(hub[k, 1] == 1.0), T["s3o_huber"].taps[k], _rel(mpf(float(c[1][0])), mpf(float(c[1][2]))) if c[1][0] != c[1][2] else 1.0)
                      for k, c in enumerate(hc)], who)
    assert x <= 2 * 3, x                                        # only the six cases one ulp off dsqr can be excused
    bad += b
    # the small solve: the pivot decision, x on the unknowns, the guard behind them
    got, lc, t = np.asarray(out["O.s3o_ldlt_solve"]).reshape(-1, 8), SC.ldlt_cases(), T["s3o_ldlt_solve"]
    bad += t.check(np.where(got[:, :1] != 0, np.concatenate([got[:, 1:7], np.where(_stack(lc, 1)[:, 37:38] == 6, 0.0, got[:, 7:8])], axis=1), 0.0), who)
    for k, c in enumerate(lc):
        if bool(got[k, 0]) == c[2]:
            bad.append("s3o_ldlt_solve/%s: %s returned %s" % (c[0], who, bool(got[k, 0])))
        if c[2] and not (got[k, 1:] == -7.0).all():
            bad.append("s3o_ldlt_solve/%s: x written by a failed solve" % c[0])
        if int(c[1][37]) == 6 and got[k, 7] != -7.0:
            bad.append("s3o_ldlt_solve/%s: x[6] written by the 6 x 6 solve" % c[0])
    return bad


def test_state_functions_on_the_host_build():
    bad = _check_O(host_outputs(), "host build")
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_state_functions_on_the_device():
    bad = _check_O(device_outputs(), "device")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------ OE. s3o_edge<1 | 2>, s3o_chi2, s3o_add_edge
J_BLOCKS = [(0, 3, 7), (3, 6, 7), (6, 7, 7), (7, 10, 7), (10, 13, 7), (13, 14, 7)]      # dP, dPhi, ds of either row
ACC_PARTS = [(0, 28, 7), (28, 35, 7), (35, 36, 7), (36, 37, 3)]                        # H, b, rho, chi2


@functools.lru_cache(maxsize=None)
def _mp_cameras():
    return [dict(ar=dict(model=c["model"], num_k=c["num_k"], fx=c["fx"], fy=c["fy"], cx=c["cx"], cy=c["cy"], dist=np.array(c["k"])),
                 Rcb=SR.V(c["Rcb"]), tcb=SR.V(c["tcb"])) for _, c, _ in SC.edge_cameras()]


def _edge_args(a):
    """(mode, camera index, 50-digit state, X, obs) of a case row"""
    return int(a[0]), int(a[1]), SR.V(a[6:9]) + SR.V(a[2:6]) + [mpf(float(a[9]))], SR.V(a[10:13]), SR.V(a[13:15])


def rst_add_edge(a):
    """s3o_chi2 and s3o_add_edge in float64, operation by operation"""
    e, J, info, delta, dsqr = [float(v) for v in a[0:2]], [float(v) for v in a[2:16]], float(a[16]), float(a[17]), float(a[18])
    chi2 = e[0] * (info * e[0]) + e[1] * (info * e[1])
    if chi2 <= dsqr:
        r0, r1 = chi2, 1.0
    else:
        sq = LM.sqrt(chi2)
        r0, r1 = 2 * sq * delta - dsqr, delta / sq
    w = r1 * info
    o0, o1 = -(info * e[0]) * r1, -(info * e[1]) * r1
    H, b = [], []
    for i in range(7):
        a0, a1 = J[i] * w, J[7 + i] * w
        H += [a0 * J[j] + a1 * J[7 + j] for j in range(i, 7)]
        b.append(J[i] * o0 + J[7 + i] * o1)
    return np.array(H + b + [r0, chi2])


@functools.lru_cache(maxsize=None)
def tables_OE():
    cs, cams, lo_cams = SC.s3o_edge_cases(), _mp_cameras(), [c for _, c, _ in SC.edge_cameras()]
    ref, rst = [], []
    for name, a in cs:
        mode, ci, st, X, obs = _edge_args(a)
        ref.append(SR.s3o_edge(mode, cams[ci], st, X, obs))
        lst = ([float(v) for v in a[6:9]], [float(v) for v in a[2:6]], float(a[9]))
        e, J = LO.edge(mode, lo_cams[ci], lst, a[10:13][None], a[13:15][None], LM)
        rst.append((e[0], J[0].reshape(-1)))
    T = {}
    for mode in (1, 2):
        rows = [k for k, c in enumerate(cs) if int(c[1][0]) == mode]
        names = [cs[k][0] for k in rows]
        T["s3o_edge<%d> e" % mode] = Table("s3o_edge<%d> e" % mode, names, [ref[k][0] for k in rows], [rst[k][0] for k in rows], [(0, 2, 7)],
                                           taps=[ref[k][2] for k in rows])
        T["s3o_edge<%d> J" % mode] = Table("s3o_edge<%d> J" % mode, names, [ref[k][1] for k in rows], [rst[k][1] for k in rows], J_BLOCKS,
                                           per_part=True)
        T["rows%d" % mode] = rows
        if mode == 2:
            # At s = 1 the ds entry is Jproj (Rcw X + tcw) = Jproj Pc, which vanishes for a projection: the 50-digit value is
            # its own residue and a relative error against it compares noise with noise.  There the entry is held to the
            # bound of the sum that cancels, 7 x 2^-52 x the sum of |products| (six products, five additions, one scaling),
            # relative to whatever the reference holds.
            tj = T["s3o_edge<2> J"]
            for k, name in enumerate(names):
                if "/s=1/" in name:
                    for part, row in ((2, 0), (5, 1)):
                        m = abs(tj.ref[k][7 * row + 6])
                        tj.floor[(k, part)] = float(7 * EPS * ref[rows[k]][2]["ds_terms"][row] / (m if m != 0 else 1))
    ac = SC.add_edge_cases()
    add = [SR.s3o_add_edge(SR.V(c[1][0:2]), SR.V(c[1][2:16]), *SR.V(c[1][16:19])) for c in ac]
    T["s3o_add_edge"] = Table("s3o_add_edge", [c[0] for c in ac], [o[0] for o in add], [rst_add_edge(c[1]) for c in ac], ACC_PARTS,
                              taps=[o[1] for o in add])
    return T


def test_edges_reference_against_restatement():
    """E_ref ceilings.  e: the image point is a float in both statements, so e is the same double unless the unrounded
    point lies within the margin of a float boundary (no case does: asserted below), and the ceiling is u.  J: every
    block is a sum of at most nine products; dPhi and ds carry the point's length over its depth, and MODE 2's ds is
    Jproj (Rcw X + tcw) (-scale^2), which is Jproj Pc = 0 at s = 1 (a projection does not see the length of its ray) and
    a (1 - scale) part of its terms elsewhere: 4096 u, and no ceiling at all for MODE 2 at s = 1, where that block is
    rounding alone (each block is held to its own E_ref on the evaluators, so the other blocks keep their bounds).  The
    accumulators: products and sums of three factors: 32 u."""
    T, bad = tables_OE(), []
    for mode in (1, 2):
        bad += ceiling_check(T["s3o_edge<%d> e" % mode], U)
        tj = T["s3o_edge<%d> J" % mode]
        bad += ceiling_check(tj, lambda k: None if mode == 2 and "/s=1/" in tj.names[k] else 4096 * U)
    bad += ceiling_check(T["s3o_add_edge"], 32 * U)
    assert not bad, "\n".join(bad)


def test_edge_cases_enter_every_branch():
    T, cs = tables_OE(), SC.s3o_edge_cases()
    A = _stack(cs, 1)
    assert set(A[:, 0]) == {1.0, 2.0} and set(A[:, 1]) == {0.0, 1.0, 2.0, 3.0} and set(A[:, 9]) == {0.5, 1.0, 2.0}
    cams = SC.edge_cameras()
    assert [c[1]["model"] for c in cams] == [0, 1, 2, 0] and any(cams[3][1]["tcb"]) and not any(cams[0][1]["tcb"])
    for mode in (1, 2):
        t = T["s3o_edge<%d> e" % mode]
        assert min(float(i["margin"]) for i in t.taps) > EXCUSE_MARGIN            # no image point on a float boundary
        z = np.array([float(i["Pc"][2]) for i in t.taps])
        for depth in (0.3, 5.0, 50.0):
            assert (np.abs(z / depth - 1) < 1e-5).any(), depth
        assert {i["kb8"] for i in t.taps} == {"-", "regular"}
        # the pinholes' border cases project onto the first or last half pixel (Radtan and KB8 move the ray's pixel)
        for k, (name, info) in enumerate(zip(t.names, t.taps)):
            a = cs[T["rows%d" % mode][k]][1]
            w, h = cams[int(a[1])][2]
            uv = [float(mpf(float(a[13 + i])) - t.ref[k][i]) for i in range(2)]
            if "border" in name and cams[int(a[1])][1]["model"] == 0:
                assert min(abs(uv[0]), abs(uv[0] - (w - 1)), abs(uv[1]), abs(uv[1] - (h - 1))) < 0.51, (name, uv)
    ad = T["s3o_add_edge"]
    assert sum(ad.taps) >= 40 and sum(not t for t in ad.taps) >= 40               # inlier and outlier edges
    assert {float(c[1][16]) for c in SC.add_edge_cases()} == {1.0, float(np.float32(1.0 / 1.2 ** 4))}


def test_edges_as_written_against_exact():
    """The Jacobian blocks as the text states them against 50-digit central differences of the unrounded error through
    the retraction (p += Rwb dp, Rwb *= Exp(dphi), s += ds), block by block, relative to the block's max-norm.  MODE 1
    is the derivative for the pinhole and the regular KB8 branch; Radtan's d(u, v) / dP leaves out the radial terms of
    k[0], k[1] (camera_radtan.h:84-90), which shows in every block.  MODE 2 is restated literally, not derived: its dP
    and ds blocks are not the derivative of this retraction (tests/test_loop_optimize.py records how they relate; the
    error does not depend on s at all there, since tcw is scaled with the point, so the derivative by s is 0 and the
    gap of ds is printed as an absolute number).  Asserted: MODE 1, and MODE 2's dPhi, with a pinhole or KB8 camera
    agree to 1e-15 (measured 5e-18: the state's quaternion is unit to a rounding only, and the retraction rotates by
    it unnormalised); everything else is printed."""
    T, cs, cams = tables_OE(), SC.s3o_edge_cases(), _mp_cameras()
    worst, bad = {}, []
    for mode in (1, 2):
        t = T["s3o_edge<%d> J" % mode]
        for k in range(0, len(t.names), 2):
            a = cs[T["rows%d" % mode][k]][1]
            m, ci, st, X, obs = _edge_args(a)
            fd = SR.s3o_edge_J_by_differences(m, cams[ci], st, X, obs)
            model = SC.edge_cameras()[ci][1]["model"]
            for bn, (lo, hi) in (("dP", (0, 3)), ("dPhi", (3, 6)), ("ds", (6, 7))):
                idx = list(range(lo, hi)) + list(range(7 + lo, 7 + hi))
                scale = max(abs(fd[i]) for i in idx)
                gap = float(max(abs(t.ref[k][i] - fd[i]) for i in idx) / (scale if scale > 1e-20 else 1))
                key = ("MODE %d" % mode, ("pinhole", "radtan", "kb8")[model], bn)
                worst[key] = max(worst.get(key, 0.0), gap)
                if (mode == 1 or bn == "dPhi") and model != 1 and not gap <= 1e-15:
                    bad.append("%s: %s of MODE 1 is %.3g from the derivative" % (t.names[k], bn, gap))
    for key in sorted(worst):
        print("s3o_edge as written against differences, %-7s %-8s %-5s %.3g" % (key + (worst[key],)))
    assert not bad, "\n".join(bad)


def _check_OE(out, who):
    T, bad = tables_OE(), []
    got = np.asarray(out["O.s3o_edge"]).reshape(-1, 18)
    for mode in (1, 2):
        rows = T["rows%d" % mode]
        te, tj = T["s3o_edge<%d> e" % mode], T["s3o_edge<%d> J" % mode]
        skip = {k for k, i in enumerate(te.taps) if i["margin"] <= EXCUSE_MARGIN}
        cap(len(skip), len(rows), "s3o_edge<%d> e" % mode)
        bad += te.check(got[rows, 0:2], who, skip=skip) + tj.check(got[rows, 2:16], who)
    if not np.array_equal(got[:, 0:2].view(np.uint64), got[:, 16:18].view(np.uint64)):
        bad.append("s3o_edge: e of the call with J == nullptr differs from e of the call with J (%s)" % who)
    ad = T["s3o_add_edge"]
    acc = np.asarray(out["O.s3o_add_edge"]).reshape(-1, 37)
    bad += ad.check(acc, who)
    ac = SC.add_edge_cases()
    b, x = decisions([("s3o_add_edge Huber/" + c[0], bool(acc[k, 35] == acc[k, 36]), ad.taps[k],
                       _rel(ad.ref[k][36], mpf(float(c[1][18])))) for k, c in enumerate(ac)], who)
    cap(x, len(ac), "s3o_add_edge")
    return bad + b


def test_edges_on_the_host_build():
    bad = _check_OE(host_outputs(), "host build")
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_edges_on_the_device():
    bad = _check_OE(device_outputs(), "device")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------ the program and the lists
def test_program_cross_compiles_for_gfx950():
    exe, log = built_program()
    assert exe is not None, log


def test_case_lists_stay_small():
    n = {k: len(v) for k, v in program_inputs().items()}
    assert all(v <= 4096 * 9 for v in n.values()), n
    assert len(SC.exp_cases()) <= 400 and len(SC.log_cases()) <= 420 and len(SC.edge_cases()) <= 200
