"""The fast single-lane forms and the one-wavefront solver of k_pose_opt_vio (csrc/vio_fast_device.h), called directly,
one lane (the solver: one workgroup) per case, and compared with the 50-digit statements of tests/algebra_ref.py on the
named cases of tests/algebra_cases.py.  tests/hip_unit/vio_fast_test.hip evaluates; nothing is compared in C++.  The
program is compiled as pose_opt_vio.hip is: the library's flags and `#pragma clang fp contract(fast)` ahead of the header.

The rule is the one of tests/test_device_algebra.py: the device's error against the as-written value is at most
4 x max(E_oracle(case), 2^-52), E_oracle the FP64 CPU oracle's error against the same value, max-norm over max-norm, part
by part where scales mix.  The oracle of the prior edge is a numpy restatement of oracle/pose_opt_vio.cc's prior_error /
prior_linearize on the oracle's own quaternion, log and JrInv hooks (tests/oracle_lib.py).

Three outputs needed a derived floor beside the rule (a rounding count of the chain x 2^-52; the derivations stand in the
docstrings of the tests that use them; none is taken from a measured device value): the rotation rows of prior_error
(8 x 2^-52 absolute; 1.07 x the bare rule on generic-41), imu_error's rows as this translation unit compiles them
(32 u S on the position and velocity rows, 26 x 2^-52 on the rotation rows; 2.26 x on
dt=0.5/zero-bias/Rij-100deg-about-y) and (chi2, err, Pc) of vis_error_flat (the ceiling tests/test_device_algebra.py
reasons for edge_error; 8.98 x on Rcb=body/rig-from-3/camera-0/depth=0.3/stereo).  In each the oracle's own error is
one sample of the same roundings and came out small; imu_error and edge_error themselves, compiled here with fused
multiply-adds, miss the bare rule on the same cases by the same factors.

Beyond the rule:
  * every domain edge is asserted from the `ok` / `w_small` the program writes, and from the inputs in 50 digits;
  * fast against plain (imu_device.h) in the same program: inside the domains within the sum of the two bounds, outside
    them the fast form hands back the plain form's bytes (every out-of-domain case of prior_error, imu_error_rot
    and ns_inc_unit);
  * prior_jacobian_init / imu_jacobian_init + a linearisation fill a buffer of NaN completely;
  * a slot that does not count leaves the 27 sums' bytes alone and yields finite values only;
  * the solver by its scaled componentwise residual rho and, where cond < 1e3, by its forward error.

Measured on an MI355X (E_oracle worst, at which case; median; the device's worst ratio to the rule's bound -- where a
floor is used: to the bare rule / to the limit with the floor; then fast against plain, of the two bounds):

  so3_exp_unit        1.3e-16 u=3/axis=111                    3.9e-17   0.20          plain 0.13
  so3_Jr_unit         2.0e-12 generic-117                     1.5e-16   0.06          plain 0.13
  q_renorm            1.5e-16 generic-30                      2.9e-17   0.31          |q|^2 - 1 = +0.99e-5: 2.8e-16,
                                                                                      -0.99e-5: 1.7e-16, bound 8.9e-16
  so3_log_unit        2.8e-16 generic-8                       7.3e-17   0.29          plain 0.21; behind q_renorm 0.39
  so3_JrInv_g         3.1e-16 outside-13                      6.7e-17   0.07          plain 0.14; g itself 0.29
  rcp_nr              1.1e-16 generic-6                       3.6e-17   0.12
  prior_error         1.1e-07 rotation-1e-9rad                6.4e-15   1.07 / 0.25   plain (e_R) 0.03
  prior_linearize     2.3e-05 state-quaternion-off-by-6e-6    2.7e-16   0.18          plain (JrInv) 0.13
  imu_error_rot       3.4e-10 residual-below-1e-5             2.6e-14   2.26 / 0.08   plain 0.15; imu_error itself 2.26
  imu_linearize_rot   3.7e-13 generic-94                      4.9e-16   0.40          plain 0.38; imu_linearize itself 0.65
  ns_inc_unit         3.2e-16 dphi-norm=7/axis=111            1.0e-16   0.35          plain 0.17
  vis_error_flat      (edge_eval<false> of test_device_algebra)         8.98 / 0.07   all 296 slots edge_error's bytes
  vis_jacobian_flat   (edge_eval<false>.J)                              0.99
  huber_flat          0.22 on the named widths, 0.25 at the edges' chi2; vis_accumulate_flat 0.24
  wave_solve_vio      rho at most 4.9e-17 (numpy 1e-17 .. 6e-16), 0.004 of its limit; forward error 0.14 of its limit
  LEAF and non-LEAF give the same bytes; identical prior and state: max |err| 2.5e-17, the Jacobian's constant
  entries exactly 0 and 1; the quaternion's norm within 1.8e-16 of 1 after one ns_inc_unit, 2.4e-16 after 1000
  excused float values: 0 of 592

Deliberate faults, each tried on a scratch copy of the header and not kept (lane cases that failed; the existing
end-to-end tests -- test_pose_opt_vio_parity, test_pose_opt_batch_narrow, test_pose_opt_vio_kat -- run on a library
built from the same scratch copy):

  the last coefficient of kAtanQ dropped      NOT caught, here or end to end (58 passed), and cannot be: the 16th term is
      (1/16)^15 / 33 = 2.6e-20 at the domain's edge, below a double's rounding of Q = 1/3 (the series carries three
      terms more than FP64 can show; test_polynomials_reproduce_the_functions pins every coefficient to the series'
      own).  Cut to 8 coefficients instead: so3_log_unit/one-ulp-inside-1/16/w>0 and /w<0 (7.4e-13 against 8.9e-16),
      w<0-inside-7, prior_error/rotation-0.4895rad, generic-3 ..., imu_error_rot/residual-0.4895rad.
  `+ 0.5 * e[2]` negated in so3_JrInv_g       so3_JrInv_g/norm/|q|^2-1=+1e-16 ... (0.106 against 8.9e-16),
      prior_linearize/rotation-0.4895rad (0.36), rotation-1e-9rad (5.2e-10), imu_linearize_rot/* (3e-3 .. 9e-3).
      End to end: every comparison with the oracle at 1e-4 passes; only test_same_bytes_as_the_parent notices (57 of 58
      pass), and it would not had the parent carried the fault.
  `+ lambda` removed from the eliminated pivots   wave_solve_vio n=15 and n=30 /lambda=1e-8-mean-diagonal (rho 4.7e-9
      against 1.3e-14), /lambda=smallest-diagonal (rho 0.09, forward error 1), /lambda=10-largest-diagonal.
      End to end: noticed where the last state is free -- test_vio_free_last_with_prior_parity[50-1500],
      test_parity_with_the_oracle[n_63_prior | n_127_prior_marg | n_600_prior_marg], test_same_bytes_as_the_parent --
      and by no other test of the three files (53 of 58 pass).
  ok left true at the Log domain test         so3_log_unit/w=0, /one-ulp-outside-1/16/w>0 and /w<0, /outside-*:
      ok is 1; prior_error/rotation-0.4905rad and rotation-3rad (e_R 1.7e36), imu_error_rot/residual-3rad,
      residual-0.4905rad, w=0.499/residual-0.4905rad (ok is 1, and not the plain forms' bytes).
      End to end: nothing notices (58 passed): no frame of those tests leaves the domains;
      tests/test_pose_opt_vio_fallback.py now does.
"""
import atexit
import functools
import math
import os
import re
import shutil
import subprocess
import tempfile

import mpmath
import numpy as np
import pytest
from mpmath import mpf

from tests import algebra_cases as AC
from tests import algebra_ref as AR
from tests import test_device_algebra as TDA
from tests.test_device_algebra import EPS, EXCUSE_CAP, EXCUSE_MARGIN, Table, U, parts_err, rel_err

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "vieo_slam_amd", "csrc", "vio_fast_device.h")
REPS = 1000               # ns_inc_unit applied this often in a row
bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.int64)


# ------------------------------------------------------------------ the stand-alone program and its files
@functools.lru_cache(maxsize=None)
def built_program():
    """(path, compiler output) of the program built into a temporary directory, or (None, output); once per session"""
    flags, hipcc = TDA.hipcc_flags()
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc") or hipcc
    d = tempfile.mkdtemp(prefix="vio_fast_")
    atexit.register(shutil.rmtree, d, True)
    exe = os.path.join(d, "vio_fast_test")
    r = subprocess.run([hipcc] + flags + ["-o", exe, os.path.join(HERE, "hip_unit", "vio_fast_test.hip")],
                       capture_output=True, text=True)
    if r.returncode != 0:
        return None, r.stdout + r.stderr
    return exe, r.stdout + r.stderr


def _stack(cases, k):
    return np.array([c[k] for c in cases], np.float64)


@functools.lru_cache(maxsize=None)
def program_inputs():
    rv, qs, rc = AC.vio_rotvec_cases(), AC.vio_quat_cases(), AC.vio_rcp_cases()
    pc, ic, nc = AC.vio_prior_cases(), AC.vio_imu_cases(), AC.vio_inc_cases()
    tab, slots = AC.vio_visual_cases()
    hc, sc = AC.vio_huber_cases(), AC.vio_solver_cases()
    H = np.zeros((len(sc), 900))
    b, x0 = np.zeros((len(sc), 32)), np.zeros((len(sc), 32))
    for k, (_, n, Hk, bk, _, _) in enumerate(sc):
        H[k, :n * n], b[k, :n] = np.asarray(Hk).reshape(-1), bk
        x0[k] = 0.5 + np.arange(32) + k
    return {
        "R.rotvec": _stack(rv, 1), "R.quat": _stack(qs, 1), "R.rcp_in": _stack(rc, 1),
        "P.prior": _stack(pc, 1), "P.state": _stack(pc, 2),
        "I.meas": _stack(ic, 1), "I.gw": _stack(ic, 2), "I.si": _stack(ic, 3), "I.sj": _stack(ic, 4),
        "N.state": _stack(nc, 1), "N.state_inc": _stack(nc, 2), "N.bias_inc": _stack(nc, 3),
        "N.reps": np.array([REPS], np.int32),
        "V.cam_f64": tab, "V.cam": np.array([s[1] for s in slots], np.int32), "V.pose": _stack(slots, 2),
        "V.obs": _stack(slots, 3), "V.valid_robust": np.array([[s[4], s[5]] for s in slots], np.int32),
        "V.delta": _stack(slots, 6), "V.acc0": _stack(slots, 7),
        "V.huber_e": _stack(hc, 1), "V.huber_delta": _stack(hc, 2), "V.huber_dsqr": _stack(hc, 3),
        "V.huber_robust": np.array([c[4] for c in hc], np.int32),
        "S.n": np.array([c[1] for c in sc], np.int32), "S.H": H, "S.b": b,
        "S.lambda": np.array([c[4] for c in sc], np.float64), "S.x0": x0,
    }


def run_program(exe):
    """("ok", outputs) or ("failed", message) of one run of a built program on the case lists"""
    d = tempfile.mkdtemp(prefix="vio_fast_run_")
    atexit.register(shutil.rmtree, d, True)
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    TDA.write_blob(fin, program_inputs())
    try:
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired as e:
        return "failed", "timed out: %s" % e
    if r.returncode != 0:
        return "failed", "exit code %d\n%s%s" % (r.returncode, r.stdout, r.stderr)
    return "ok", TDA.read_blob(fout)


@functools.lru_cache(maxsize=None)
def device_run():
    """the program is built once, fed once and run once; a failure is cached and every test reports it without
    starting the program again"""
    exe, log = built_program()
    if exe is None:
        return "failed", "hipcc failed:\n" + log
    return run_program(exe)


def device_outputs():
    st, out = device_run()
    assert st == "ok", out
    return out


def _oracle():
    from tests import oracle_lib
    return oracle_lib.load()


def check_floor(t, dev, floor, skip=(), indexed=False):
    """The rule with a derived floor beside it, part by part: error <= max(4 x max(E_oracle(case), 2^-52),
    floor(case, part)), the floor a rounding count of the chain x 2^-52 over the part's max-norm (the derivations stand
    at the callers).  Prints the worst ratio to the rule alone and to the limit used."""
    dev = np.asarray(dev).reshape(len(t.names), -1)
    bad, worst_rule, worst = [], 0.0, 0.0
    for k, name in enumerate(t.names):
        if name in skip:
            continue
        for pi, (a, b) in enumerate(t.parts):
            e = rel_err(dev[k, a:b], t.ref[k][a:b])
            lim = max(t.bound(k), floor(k, pi))
            worst_rule, worst = max(worst_rule, e / t.bound(k)), max(worst, e / lim)
            if not e <= lim:
                bad.append((k, "%s/%s[%d:%d]: error %.3g, limit %.3g (the rule %.3g, floor %.3g)" % (
                    t.fn, name, a, b, e, lim, t.bound(k), floor(k, pi))))
    print("%-22s device worst ratio to the rule %.3f, to the limit with its floor %.3f" % (t.fn, worst_rule, worst))
    return bad if indexed else [m for _, m in bad]


def fast_vs_plain(fn, names, fast, plain, ref, bound, inside, parts=None, only=None):
    """inside the domain: |fast - plain| within the sum of the two bounds (each bound(k) of the reference's max-norm);
    outside: the same bytes.  only = "inside" / "outside": the other cases are left to another test."""
    bad, worst = [], 0.0
    fast, plain = np.asarray(fast).reshape(len(names), -1), np.asarray(plain).reshape(len(names), -1)
    for k, name in enumerate(names):
        if only is not None and (only == "inside") != bool(inside[k]):
            continue
        if inside[k]:
            for a, b in (parts or [(0, fast.shape[1])]):
                m = float(max(abs(t) for t in ref[k][a:b]))
                d = float(np.abs(fast[k, a:b] - plain[k, a:b]).max()) / (m if m else 1.0)
                worst = max(worst, d / (2 * bound(k)))
                if not d <= 2 * bound(k):
                    bad.append("%s/%s: fast and plain differ by %.3g, the two bounds are %.3g" % (fn, name, d, 2 * bound(k)))
        elif not (bits(fast[k]) == bits(plain[k])).all():
            bad.append("%s/%s: outside the domain, but not the plain form's bytes" % (fn, name))
    print("%-22s fast against plain, worst ratio to the two bounds %.3f" % (fn, worst))
    return bad


# ------------------------------------------------------------------ the header's constants
@functools.lru_cache(maxsize=None)
def header_constants():
    text = open(HEADER).read()
    out = {}
    for name in ("kCosH", "kSinHT", "kJrA", "kJrB", "kAtanQ"):
        m = re.search(r"constexpr double %s\[(\d+)\] = \{([^}]*)\};" % name, text)
        assert m, name
        out[name] = [float(t) for t in m.group(2).split(",")]
        assert len(out[name]) == int(m.group(1))
    return out


def _poly(c, u):
    r = mpf(0)
    for t in reversed(c):
        r = r * u + mpf(t)
    return r


def test_polynomials_reproduce_the_functions():
    """As written against exact.  With the header's double coefficients, evaluated in 50 digits, the polynomials give
    cos(t / 2), sin(t / 2) / t, A = (1 - cos t) / t^2, B = (t - sin t) / t^3 on u = t^2 <= 1 / 4 and P = atan(x) / x,
    g = Q / (4 P^2) on x^2 <= 1 / 16 to below 2^-53, the domain's edge included; every coefficient is the series' own
    rounded to double; and g = Q / (4 P^2) is (1 - t (1 + cos t) / (2 sin t)) / t^2 at t = 2 atan x."""
    K = header_constants()
    fact = mpmath.factorial
    series = {"kCosH": lambda k: mpf(-1) ** k / (mpf(4) ** k * fact(2 * k)),
              "kSinHT": lambda k: mpf(-1) ** k / (2 * mpf(4) ** k * fact(2 * k + 1)),
              "kJrA": lambda k: mpf(-1) ** k / fact(2 * k + 2), "kJrB": lambda k: mpf(-1) ** k / fact(2 * k + 3),
              "kAtanQ": lambda k: mpf(-1) ** k / (2 * k + 3)}
    for name, f in series.items():
        for k, c in enumerate(K[name]):
            assert c == float(f(k)), (name, k)
        # the first omitted term at the domain's edge: below 1e-17, as the header says
        edge = mpf(1) / 4 if name != "kAtanQ" else mpf(1) / 16
        assert abs(f(len(K[name]))) * edge ** len(K[name]) < 1e-17, name
    worst = {}

    def see(what, got, want):
        worst[what] = max(worst.get(what, 0.0), float(abs(got - want)))
    us = [mpf(0), mpf(1e-20)] + [mpf(0.25) * k / 32 for k in range(1, 33)] + [mpf(float(np.nextafter(0.25, 0)))]
    for u in us:
        t = mpmath.sqrt(u)
        see("cos(t/2)", _poly(K["kCosH"], u), mpmath.cos(t / 2))
        see("sin(t/2)/t", _poly(K["kSinHT"], u), mpmath.sin(t / 2) / t if t else mpf(1) / 2)
        see("A", _poly(K["kJrA"], u), (1 - mpmath.cos(t)) / u if t else mpf(1) / 2)
        see("B", _poly(K["kJrB"], u), (t - mpmath.sin(t)) / (t * u) if t else mpf(1) / 6)
    for x2 in [u / 4 for u in us]:
        P_ex, Q_ex = AR.atan_PQ_ex(x2)
        Q = _poly(K["kAtanQ"], x2)
        P = 1 - x2 * Q
        see("atan(x)/x", P, P_ex)
        see("Q", Q, Q_ex)
        t = 2 * mpmath.atan(mpmath.sqrt(x2))
        see("g", Q / (4 * P * P), AR.jrinv_g_ex(t))
        see("g = Q/(4P^2), exact", Q_ex / (4 * P_ex * P_ex), AR.jrinv_g_ex(t))
    for what, g in worst.items():
        print("%-22s polynomial against exact, worst gap %.3g" % (what, g))
        assert g < (1e-45 if "exact" in what else 2.0 ** -53), (what, g)


# ------------------------------------------------------------------ R. rotations
@functools.lru_cache(maxsize=None)
def tables_R():
    O = _oracle()
    rv, qs, rc = AC.vio_rotvec_cases(), AC.vio_quat_cases(), AC.vio_rcp_cases()
    n_rv, n_q = [c[0] for c in rv], [c[0] for c in qs]
    T = {}
    T["so3_exp_unit"] = Table("so3_exp_unit", n_rv, [AR.so3_exp_aw(AR.V(c[1])) for c in rv], [O.so3_exp(c[1]) for c in rv])
    T["so3_Jr_unit"] = Table("so3_Jr_unit", n_rv, [AR.so3_Jr_aw(AR.V(c[1])) for c in rv],
                             [O.so3_jr(c[1]).reshape(-1) for c in rv])
    T["q_renorm"] = Table("q_renorm", n_q, [AR.q_norm(AR.V(c[1])) for c in qs], [O.quat_normalize(c[1]) for c in qs])
    logs = [AR.so3_log_aw(AR.V(c[1])) for c in qs]
    T["so3_log_unit"] = Table("so3_log_unit", n_q, logs, [O.so3_log(c[1]) for c in qs])
    T["so3_JrInv_g"] = Table("so3_JrInv_g", n_q, [AR.so3_JrInv_aw(l) for l in logs],
                             [O.so3_jr(O.so3_log(c[1]), inverse=True).reshape(-1) for c in qs])
    # behind q_renorm / q_norm: the log of the normalised quaternion
    T["so3_log_unit.renorm"] = Table("so3_log_unit.renorm", n_q, [AR.so3_log_aw(AR.q_norm(AR.V(c[1]))) for c in qs],
                                     [O.so3_log(O.quat_normalize(c[1])) for c in qs])
    T["rcp_nr"] = Table("rcp_nr", [c[0] for c in rc], [[1 / mpf(c[1])] for c in rc], [np.array([1.0 / c[1]]) for c in rc])
    return T


def _g_of(J_ref_log):
    """the exact g of JrInv(e) = I + hat(e) / 2 + g hat(e)^2 (below 1e-5 rad the reference takes 1 / 12, which is off by
    t^2 / 60 of g and by nothing that shows in the matrix)"""
    return AR.jrinv_g_ex(AR.norm3(J_ref_log))


def test_rotation_cases_sit_on_their_side():
    """from the inputs, in 50 digits: which side of u < 1 / 4, n^2 < w^2 / 16 and ||q|^2 - 1| < 1e-5 a case is on"""
    for name, w, inside in AC.vio_rotvec_cases():
        u = sum(t * t for t in AR.V(w))
        assert (u < mpf(0.25)) == inside, name
        if "one-ulp-below" in name:
            assert max(abs(w)) == AC.HALF_BELOW and np.count_nonzero(w) == 1
        if "one-ulp-above" in name:
            assert max(abs(w)) == AC.HALF_ABOVE and np.count_nonzero(w) == 1
    us = [float(np.dot(c[1], c[1])) for c in AC.vio_rotvec_cases()]
    assert 0.0 in us and any(0 < u < 1e-19 for u in us) and any(abs(u - 0.3) < 1e-15 for u in us) and any(abs(u - 3) < 1e-14 for u in us)
    seen = set()
    for name, q, inside, e in AC.vio_quat_cases():
        q = AR.V(q)
        n2, w2 = q[1] ** 2 + q[2] ** 2 + q[3] ** 2, q[0] ** 2
        assert (n2 < w2 / 16) == inside, name
        if name.startswith("one-ulp"):     # adjacent doubles, and the rounded products decide as the exact ones do
            assert float(q[2]) == 0 and float(q[3]) == 0
            seen.add(name)
        if e is not None:
            ex = n2 + w2 - 1
            assert abs(ex - mpf(e)) < 1e-15 and (abs(ex) < mpf(1e-5)) == (abs(e) < 1e-5), (name, ex)
    qs = {c[0]: c[1] for c in AC.vio_quat_cases()}
    for s in ("w>0", "w<0"):
        a, b = qs["one-ulp-inside-1/16/" + s], qs["one-ulp-outside-1/16/" + s]
        assert b[1] == np.nextafter(a[1], 1.0) and a[0] == b[0] and (a[0] < 0) == (s == "w<0")
    assert len(seen) == 4 and any(c[1][0] < 0 and c[2] for c in AC.vio_quat_cases())


@pytest.mark.gpu
def test_rotations_on_the_device():
    out, T, bad = device_outputs(), tables_R(), []
    rv, qs = AC.vio_rotvec_cases(), AC.vio_quat_cases()
    ex = out["R.so3_exp_unit"].reshape(-1, 5)
    inside = [c[2] for c in rv]
    for k, c in enumerate(rv):                    # the domain test, from the program's own ok
        if bool(ex[k, 4]) != c[2]:
            bad.append("so3_exp_unit/%s: ok is %d" % (c[0], ex[k, 4]))
    out_names = tuple(c[0] for c in rv if not c[2])
    bad += T["so3_exp_unit"].check_device(ex[:, :4], skip=out_names)
    bad += T["so3_Jr_unit"].check_device(out["R.so3_Jr_unit"], skip=out_names)
    # fast against plain inside the domain (so3_exp_unit and so3_Jr_unit have no fallback of their own)
    bad += fast_vs_plain("so3_exp_unit", [c[0] for c in rv if c[2]], ex[inside][:, :4], out["R.so3_exp_q"].reshape(-1, 4)[inside],
                         [r for r, i in zip(T["so3_exp_unit"].ref, inside) if i],
                         lambda k, B=[T["so3_exp_unit"].bound(j) for j in range(len(rv)) if inside[j]]: B[k], [True] * sum(inside))
    bad += fast_vs_plain("so3_Jr_unit", [c[0] for c in rv if c[2]], out["R.so3_Jr_unit"].reshape(-1, 9)[inside],
                         out["R.so3_Jr_d"].reshape(-1, 9)[inside], [r for r, i in zip(T["so3_Jr_unit"].ref, inside) if i],
                         lambda k, B=[T["so3_Jr_unit"].bound(j) for j in range(len(rv)) if inside[j]]: B[k], [True] * sum(inside))
    # q_renorm: ok flips between |q|^2 - 1 = 0.99e-5 and 1.01e-5; inside, the value is q_norm's by the rule
    rn = out["R.q_renorm"].reshape(-1, 5)
    unit = [c[3] is None or abs(c[3]) < 1e-5 for c in qs]
    for k, c in enumerate(qs):
        if bool(rn[k, 4]) != unit[k]:
            bad.append("q_renorm/%s: ok is %d" % (c[0], rn[k, 4]))
    bad += T["q_renorm"].check_device(rn[:, :4], skip=tuple(c[0] for c, u in zip(qs, unit) if not u))
    for k, c in enumerate(qs):
        if c[3] is not None and abs(c[3]) < 1e-5:
            e = parts_err(rn[k, :4], T["q_renorm"].ref[k], [(0, 4)])
            print("q_renorm/%s: error %.3g, bound %.3g" % (c[0], e, T["q_renorm"].bound(k)))
    # so3_log_unit and g on the quaternion as given: ok from the program, values inside the domain by the rule
    lg, lc = out["R.so3_log_unit"].reshape(-1, 5), out["R.so3_log_unit.renorm"].reshape(-1, 5)
    for k, c in enumerate(qs):
        if bool(lg[k, 4]) != c[2]:
            bad.append("so3_log_unit/%s: ok is %d" % (c[0], lg[k, 4]))
        if bool(lc[k, 4]) != (c[2] and unit[k]):
            bad.append("so3_log_unit behind q_renorm/%s: ok is %d" % (c[0], lc[k, 4]))
    outside = tuple(c[0] for c in qs if not c[2])
    bad += T["so3_log_unit"].check_device(lg[:, :3], skip=outside)
    bad += T["so3_log_unit.renorm"].check_device(lc[:, :3], skip=tuple(c[0] for c, u in zip(qs, unit) if not (c[2] and u)))
    bad += T["so3_JrInv_g"].check_device(out["R.so3_JrInv_g"], skip=outside)
    worst = 0.0
    O = _oracle()
    for k, c in enumerate(qs):                    # g itself, relative: the rule with the closed form in FP64 as the oracle
        if not c[2]:
            continue
        g_ref = _g_of(T["so3_log_unit"].ref[k])
        t = float(np.linalg.norm(O.so3_log(c[1])))
        g_or = 1. / 12. if t < 1e-5 else (1.0 - (1.0 + math.cos(t)) * t / (2.0 * math.sin(t))) / (t * t)
        e_or = float(abs(mpf(g_or) - g_ref) / g_ref)
        e = float(abs(mpf(float(lg[k, 3])) - g_ref) / g_ref)
        worst = max(worst, e / (4 * max(e_or, EPS)))
        if not e <= 4 * max(e_or, EPS):
            bad.append("g/%s: error %.3g, the closed form's in FP64 %.3g" % (c[0], e, e_or))
    print("%-22s device worst ratio to its bound %.3f" % ("g of so3_log_unit", worst))
    if not (bits(out["R.so3_JrInv_g_of"].reshape(-1, 2)[:, 0]) == bits(out["R.so3_JrInv_g_of"].reshape(-1, 2)[:, 1]))[[c[1][0] != 0 for c in qs]].all():
        bad.append("so3_JrInv_g_of and its inlined twin differ")
    ins = [c[2] for c in qs]
    nm = [c[0] for c in qs if c[2]]
    bad += fast_vs_plain("so3_log_unit", nm, lg[ins][:, :3], out["R.so3_log_q"].reshape(-1, 3)[ins],
                         [r for r, i in zip(T["so3_log_unit"].ref, ins) if i],
                         lambda k, B=[T["so3_log_unit"].bound(j) for j in range(len(qs)) if ins[j]]: B[k], [True] * len(nm))
    bad += fast_vs_plain("so3_JrInv_g", nm, out["R.so3_JrInv_g"].reshape(-1, 9)[ins], out["R.so3_JrInv_d"].reshape(-1, 9)[ins],
                         [r for r, i in zip(T["so3_JrInv_g"].ref, ins) if i],
                         lambda k, B=[T["so3_JrInv_g"].bound(j) for j in range(len(qs)) if ins[j]]: B[k], [True] * len(nm))
    # negative q.w inside the domain: the same vector as the plain so3_log_q, by the rule (above) -- and as Log(-q)
    bad += T["rcp_nr"].check_device(out["R.rcp_nr"])
    assert not bad, "\n".join(bad[:60])


# ------------------------------------------------------------------ P. the prior edge
PRIOR_PARTS = [(0, 3), (3, 6), (6, 9), (9, 12), (12, 15)]


def _full_state(s):
    return {"p": AR.V(s[0:3]), "v": AR.V(s[3:6]), "q": AR.V(s[6:10]), "bg": AR.V(s[10:13]), "ba": AR.V(s[13:16]),
            "dbg": AR.V(s[16:19]), "dba": AR.V(s[19:22])}


def oracle_prior(O, pr, si):
    """oracle/pose_opt_vio.cc prior_error / prior_linearize restated on the oracle's hooks: err[15], J[15 x 15]"""
    Rb = O.quat_to_R(pr[6:10]).reshape(3, 3)
    err = np.zeros(15)
    err[0:3] = Rb.T @ (si[0:3] - pr[0:3])
    qc = pr[6:10] * np.array([1.0, -1, -1, -1])
    err[6:9] = O.so3_log(O.quat_normalize(O.quat_mul(qc, si[6:10])))
    err[3:6] = si[3:6] - pr[3:6]
    err[9:12] = si[10:13] + si[16:19] - (pr[10:13] + pr[16:19])
    err[12:15] = si[13:16] + si[19:22] - (pr[13:16] + pr[19:22])
    J = np.zeros((15, 15))
    J[0:3, 0:3] = Rb.T @ O.quat_to_R(si[6:10]).reshape(3, 3)
    J[3:6, 3:6] = J[9:12, 9:12] = J[12:15, 12:15] = np.eye(3)
    J[6:9, 6:9] = O.so3_jr(err[6:9], inverse=True)
    return err, J.reshape(-1)


@functools.lru_cache(maxsize=None)
def tables_P():
    O = _oracle()
    pc = AC.vio_prior_cases()
    names, eref, jref, eor, jor = [c[0] for c in pc], [], [], [], []
    for name, pr, si, ok in pc:
        a, b = _full_state(pr), _full_state(si)
        e = [mpf(0) if abs(t) < mpf(10) ** -40 else t for t in AR.prior_error_aw(a, b)]    # (the 50 digits' own noise)
        eref.append(e), jref.append(AR.prior_linearize_aw(a, b, e))
        oe, oj = oracle_prior(O, pr, si)
        eor.append(oe), jor.append(oj)
    return {"prior_error": Table("prior_error", names, eref, eor, PRIOR_PARTS),
            "prior_linearize": Table("prior_linearize", names, jref, jor)}


def test_prior_reference_against_oracle():
    """E_oracle ceilings, reasoned as for the inertial edge: e_p rotates a difference of positions of up to 10 m that
    cancels to centimetres: 32 u S / |e_p|; e_v and the bias rows are one or three roundings of terms that cancel:
    8 u S / |row|; e_R is the log of a normalised product of two unit quaternions: 64 u / |e_R|.  The Jacobian is a
    product of two rotation matrices, identities and JrInv(e_R): 64 u (1 + th / |sin th|)."""
    T, bad = tables_P(), []
    pc = AC.vio_prior_cases()

    def err_ceiling(k):
        _, pr, si, _ = pc[k]
        r = [float(max(abs(t) for t in T["prior_error"].ref[k][a:b])) for a, b in PRIOR_PARTS]
        S = [3 * (np.abs(pr[0:3]).max() + np.abs(si[0:3]).max() + 1), np.abs(pr[3:6]).max() + np.abs(si[3:6]).max() + 1, 4.0,
             1.0, 1.0]
        c = [32 * U * S[0], 8 * U * S[1], 64 * U * S[2], 8 * U, 8 * U]
        return max(ci / ri if ri else ci for ci, ri in zip(c, r))

    def J_ceiling(k):
        if pc[k][0].startswith("state-quaternion"):      # the oracle takes R of the quaternion as stored, off by |q|^2 - 1
            return None
        th = float(AR.norm3(T["prior_error"].ref[k][6:9]))
        return 64 * U * (1 + (th / abs(math.sin(th)) if th >= 1e-5 else 1))
    bad += TDA.ceiling_check(T["prior_error"], err_ceiling)
    bad += TDA.ceiling_check(T["prior_linearize"], J_ceiling)
    assert not bad, "\n".join(bad)


def test_prior_as_written_against_exact():
    """The residual with SO3ex's closed-form log against the exact log (1e-15), and linearizeOplus against central
    differences (h = 1e-15 under 50 digits) of the exact residual over the vertices' retraction (p + R dp, v + dv,
    R Exp(dphi), bias + db): every block is the first-order derivative, so 1e-20 of the max-norm, the accuracy
    tests/test_device_algebra.py pins for imu_linearize.  Identical prior and state: err = 0 and identity blocks."""
    worst_e = worst_J = 0.0
    done = 0
    for name, pr, si, ok in AC.vio_prior_cases():
        a, b = _full_state(pr), _full_state(si)
        a["q"], b["q"] = AR.q_norm(a["q"]), AR.q_norm(b["q"])
        e_aw, e_ex = AR.prior_error_aw(a, b), AR.prior_error_ex(a, b)
        ge = float(max(abs(x - y) for x, y in zip(e_aw, e_ex)))
        worst_e = max(worst_e, ge)
        assert ge <= 1e-15, (name, ge)
        if name == "identical":
            J = AR.prior_linearize_aw(a, b, e_aw)
            assert all(abs(t) < 1e-45 for t in e_aw)
            assert all(abs(J[r * 15 + c] - (1 if r == c else 0)) < 1e-45 for r in range(15) for c in range(15))
        if done >= 12 and not name.startswith(("rotation", "identical")):
            continue
        done += 1
        J = AR.prior_linearize_aw(a, b, e_ex)
        h, gJ = AR.H_FD, 0
        for c in range(15):
            es = []
            for sgn in (1, -1):
                bb = dict(b)
                if c < 9:
                    d = [mpf(0)] * 9
                    d[c] = sgn * h
                    bb.update(TDA._retract(b, d, 6))
                else:
                    key, j = ("dbg", c - 9) if c < 12 else ("dba", c - 12)
                    bb[key] = list(b[key])
                    bb[key][j] += sgn * h
                es.append(AR.prior_error_ex(a, bb))
            for r in range(15):
                gJ = max(gJ, abs((es[0][r] - es[1][r]) / (2 * h) - J[r * 15 + c]))
        gJ = float(gJ / max(abs(t) for t in J))
        worst_J = max(worst_J, gJ)
        assert gJ <= 1e-20, (name, gJ)
    print("prior_error            as written against exact, worst gap %.3g" % worst_e)
    print("prior_linearize        as written against central differences, worst gap %.3g over %d cases" % (worst_J, done))


def _eR_floor(t, rows, count):
    """count x 2^-52 absolute on the rotation rows, over their max-norm"""
    def floor(k, pi):
        if t.parts[pi] != rows:
            return 0.0
        m = float(max(abs(x) for x in t.ref[k][rows[0]:rows[1]]))
        return count * EPS / m if m else count * EPS
    return floor


@pytest.mark.gpu
def test_prior_edge_on_the_device():
    """A derived floor stands beside the rule on the rotation rows (the oracle's own error is one sample of the same
    roundings, and a sample can be lucky: generic-41, a residual rotation of 1e-6 rad, came out at 4.3 x E_oracle).

    e_R = Log(renorm(conj(q_prior) q_i)): a component of the product is four products and three sums of partial sums
    bounded by sum |a_i b_j| <= 1: at most 4 u absolute; q_renorm multiplies by a factor good to 2 u; so3_log_unit
    scales by f = 2 P / w (about 2, good to 5 u).  In all 2 (4 u + 2 u) + 5 u |e_R| <= 14.5 u: 8 x 2^-52 absolute."""
    out, T, bad = device_outputs(), tables_P(), []
    pc = AC.vio_prior_cases()
    n = len(pc)
    ok, plain = out["P.ok"], out["P.plain"].reshape(n, 17)
    for k, c in enumerate(pc):
        if bool(ok[k]) != c[3]:
            bad.append("prior_error/%s: ok is %d" % (c[0], ok[k]))
    for tag in ("", "<LEAF>"):
        err, J = out["P.prior_error" + tag].reshape(n, 15), out["P.prior_jacobian" + tag].reshape(n, 225)
        cache = out["P.cache" + tag].reshape(n, 5)
        bad += check_floor(T["prior_error"], err, _eR_floor(T["prior_error"], (6, 9), 8))
        if not np.isfinite(J).all():
            bad.append("prior_jacobian%s: the buffer of NaN is not filled" % tag)
        bad += T["prior_linearize"].check_device(J)
        # the constant part is exact
        const = np.ones((15, 15), bool)
        const[0:3, 0:3] = const[6:9, 6:9] = False
        want = np.diag([0.0] * 3 + [1.0] * 3 + [0.0] * 3 + [1.0] * 6)
        if not (J.reshape(n, 15, 15)[:, const] == want[const]).all():
            bad.append("prior_jacobian%s: a constant entry is not 0 or 1" % tag)
        bad += fast_vs_plain("prior_error%s e_R" % tag, [c[0] for c in pc], err[:, 6:9], plain[:, 4:7],
                             [r[6:9] for r in T["prior_error"].ref], T["prior_error"].bound, [c[3] for c in pc])
        # the cache: a unit quaternion within 4 x 2^-52 per form inside the domain (g is compared through the Jacobian);
        # outside, quaternion and g are the plain forms' bytes
        bad += fast_vs_plain("prior cache%s" % tag, [c[0] for c in pc], cache, np.hstack([plain[:, 0:4], plain[:, 7:8]]),
                             [[mpf(1)] * 5] * n, lambda k: 4 * EPS, [c[3] for c in pc], [(0, 4)])
        bad += fast_vs_plain("prior JrInv%s" % tag, [c[0] for c in pc], J.reshape(n, 15, 15)[:, 6:9, 6:9].reshape(n, 9), plain[:, 8:17],
                             [AR.so3_JrInv_aw(r[6:9]) for r in T["prior_error"].ref], T["prior_linearize"].bound, [True] * n)
    k = [c[0] for c in pc].index("identical")
    e = out["P.prior_error"].reshape(n, 15)[k]
    print("prior_error/identical  max |err| %.3g" % np.abs(e).max())
    assert not bad, "\n".join(bad[:60])


# ------------------------------------------------------------------ I. the inertial edge
@functools.lru_cache(maxsize=None)
def tables_I():
    from vieo_slam_amd.ba_types import VIO_FRAME_DTYPE
    O = _oracle()
    TE = TDA.tables_E()
    idx = {nm: k for k, nm in enumerate(TE["imu_error"].names)}
    names, eref, jref, eor, jor = [], [], [], [], []
    for name, M, gw, si, sj, ok, ws in AC.vio_imu_cases():
        names.append(name)
        k = idx.get(name + "/PVR")
        if k is not None:
            eref.append(TE["imu_error"].ref[k]), jref.append(TE["imu_linearize"].ref[k])
            eor.append(TE["imu_error"].orc[k]), jor.append(TE["imu_linearize"].orc[k])
            continue
        md, a, b = TDA._meas_dict(M), TDA._state_dict(si), TDA._state_dict(sj)
        e = AR.imu_error_aw(md, AR.V(gw), a, b, 6)
        eref.append(e), jref.append(AR.imu_linearize_aw(md, AR.V(gw), a, b, e, 6))
        F = np.zeros(1, VIO_FRAME_DTYPE)
        for key, lo, hi in TDA.M_FIELDS:
            F["imu"][key] = M[lo] if key == "dt" else M[lo:hi]
        F["gw"] = gw
        oe, Ji, Jj, JB = O.imu_edge_eval(F, TDA._navstate(si), TDA._navstate(sj))
        eor.append(oe.copy()), jor.append(np.hstack([Jj, Ji, JB]).reshape(-1))
    return {"imu_error": Table("imu_error_rot", names, eref, eor, TDA.ERR_PARTS),
            "imu_linearize": Table("imu_linearize_rot", names, jref, jor)}


def test_inertial_cases_sit_on_their_side():
    """from the inputs in 50 digits: |JgR dbg|^2 against 1 / 4, the as-written residual rotation against
    2 atan(1 / 4), the state quaternions' norms against 1e-5"""
    T = tables_I()
    seen = set()
    for k, (name, M, gw, si, sj, ok, ws) in enumerate(AC.vio_imu_cases()):
        w = AR.mv3(AR.V(M[16:25]), AR.V(si[16:19]))
        u = sum(t * t for t in w)
        th = AR.norm3(T["imu_error"].ref[k][6:9])
        n2 = [sum(t * t for t in AR.V(s[6:10])) for s in (si, sj)]
        unit = abs(n2[0] * n2[1] - 1) < mpf(1e-5)            # |conj(q_i) q_j|^2 - 1, which q_renorm tests
        assert (u < mpf(0.25)) == ws, name
        assert (ws and unit and th < mpf(AC.LOG_EDGE) * (1 - mpf(10) ** -9)) == ok, (name, th)
        assert abs(th - mpf(AC.LOG_EDGE)) > 1e-6 and abs(u - mpf(0.25)) > 1e-6      # no case leaves the side to rounding
        seen.add((ok, ws))
        if name.startswith("w=0.499"):
            assert 0.24 < u < 0.25
        if name.startswith("w=0.501"):
            assert 0.25 < u < 0.26
        if "residual-0.4895" in name or "residual-0.4905" in name:
            assert abs(th - mpf(name.split("residual-")[1][:6])) < 1e-3
    assert seen == {(True, True), (False, True), (False, False)}


@pytest.mark.gpu
def test_inertial_edge_on_the_device():
    """Derived floors beside the rule (dt=0.5/zero-bias/Rij-100deg-about-y came out at 9 x E_oracle -- imu_error itself
    does, as this translation unit compiles it, so the floor is not one of the fast forms alone).

    Position and velocity rows: differences of terms of size S that cancel to millimetres, an absolute error of 32 u S
    (the count tests/test_device_algebra.py pins for this chain in test_inertial_reference_against_oracle).

    e_R = Log(renorm(conj(qa) qb)), qa = renorm(qRij qx), qb = renorm(conj(q_i) q_j): R_to_q leaves 4 u per component,
    so3_exp_unit 3 u; a product adds its factors' errors and 4 u of its own, q_renorm 2 u: qa 13 u, qb 6 u, qe 25 u;
    so3_log_unit doubles that and adds 5 u |e_R|: 52.5 u, i.e. 26 x 2^-52 absolute (rounded down)."""
    out, T, bad = device_outputs(), tables_I(), []
    ic = AC.vio_imu_cases()
    n = len(ic)
    names = [c[0] for c in ic]
    tE = T["imu_error"]
    eR = _eR_floor(tE, (6, 9), 26)

    def err_floor(k, pi):
        if pi == 2:
            return eR(k, pi)
        _, M, gw, si, sj, _, _ = ic[k]
        S = TDA._imu_scale(M, gw, si, sj)[pi]
        m = float(max(abs(x) for x in tE.ref[k][3 * pi:3 * pi + 3]))
        return 32 * U * S / m if m else 32 * U * S
    ok, pq = out["I.ok"].reshape(n, 2), out["I.plain"].reshape(n, 9)
    for k, c in enumerate(ic):
        if (bool(ok[k, 0]), bool(ok[k, 1])) != (c[5], c[6]):
            bad.append("imu_error_rot/%s: (ok, w_small) is (%d, %d)" % (c[0], ok[k, 0], ok[k, 1]))
    perr, pJ = out["I.imu_error"].reshape(n, 9), out["I.imu_linearize"].reshape(n, 216)
    bad += check_floor(tE, perr, err_floor)          # the plain forms as this translation unit compiles them
    bad += T["imu_linearize"].check_device(pJ)
    for tag in ("", "<LEAF>"):
        err, J = out["I.imu_error_rot" + tag].reshape(n, 9), out["I.jacobian" + tag].reshape(n, 216)
        cache = out["I.cache" + tag].reshape(n, 13)
        if not (cache[:, 12] == ok[:, 1]).all():
            bad.append("imu_error_rot%s: the cache's w_small is not the chain's" % tag)
        bad += check_floor(tE, err, err_floor)
        if not np.isfinite(J).all():
            bad.append("imu jacobian%s: the buffer of NaN is not filled" % tag)
        bad += T["imu_linearize"].check_device(J)
        inside = [c[5] for c in ic]
        # (outside the domain, the bytes: test_inertial_fallback_hands_back_the_plain_forms_bytes)
        bad += fast_vs_plain("imu_error_rot%s" % tag, names, err, perr, T["imu_error"].ref, T["imu_error"].bound, [True] * n,
                             TDA.ERR_PARTS)
        bad += fast_vs_plain("imu cache%s" % tag, names, cache[:, :9], pq, [[mpf(1)] * 9] * n, lambda k: 4 * EPS, [True] * n,
                             [(0, 4), (4, 8)])
        bad += fast_vs_plain("imu jacobian%s" % tag, names, J, pJ, T["imu_linearize"].ref, T["imu_linearize"].bound, [True] * n)
    J0, J1 = out["I.jacobian"].reshape(n, 216), out["I.jacobian.part1"].reshape(n, 216)
    # the four-wavefront instances' init + pv + rot against the one-wavefront instances' imu_linearize part 1 + rot: the same
    # values (set3 writes the zeros of -I as -1.0 x 0 = -0.0, imu_jacobian_init as 0.0: equal, not the same bytes)
    if not (J0 == J1).all():
        k = int(np.flatnonzero((J0 != J1).any(1))[0])
        bad.append("imu jacobian/%s: init + pv + rot differs from imu_linearize part 1 + rot" % names[k])
    if not (bits(out["I.imu_error_rot"]) == bits(out["I.imu_error_rot<LEAF>"])).all():
        print("imu_error_rot          LEAF and non-LEAF differ in bytes")
    assert not bad, "\n".join(bad[:60])


@pytest.mark.gpu
def test_inertial_fallback_hands_back_the_plain_forms_bytes():
    """Outside the domains imu_error_rot's rotation rows are imu_error's bytes, and its cache (qe, qb, g) the bytes of
    the plain chain and of so3_JrInv_g_of: all six cases, both LEAF forms.

    This holds because the program calls every form under test and the plain forms as out-of-line functions of their
    own.  Under `fp contract(fast)` the compiler fuses a * b + c per context; with all of them inlined into one kernel
    they shared common subexpressions, the fallback's products gained second uses and were fused otherwise, and
    w=0.501/residual-small differed from imu_error by 7.4e-17 rad.  k_pose_opt_vio holds no second copy of the plain
    chain beside its fallback either."""
    out, T, bad = device_outputs(), tables_I(), []
    ic = AC.vio_imu_cases()
    n = len(ic)
    names, inside = [c[0] for c in ic], [c[5] for c in ic]
    assert inside.count(False) == 6
    perr, pq = out["I.imu_error"].reshape(n, 9), out["I.plain"].reshape(n, 9)
    for tag in ("", "<LEAF>"):
        err, cache = out["I.imu_error_rot" + tag].reshape(n, 9), out["I.cache" + tag].reshape(n, 13)
        bad += fast_vs_plain("imu_error_rot%s" % tag, names, err, perr, T["imu_error"].ref, T["imu_error"].bound, inside,
                             only="outside")
        bad += fast_vs_plain("imu cache%s" % tag, names, cache[:, :9], pq, None, None, inside, only="outside")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------ N. the retraction
@functools.lru_cache(maxsize=None)
def tables_N():
    O = _oracle()
    nc = AC.vio_inc_cases()
    ref, orc = [], []
    for name, s, d9, db, ok in nc:
        p, v, q, dbg, dba = AR.ns_inc_aw(AR.V(s[0:3]), AR.V(s[3:6]), AR.V(s[6:10]), AR.V(s[16:19]), AR.V(s[19:22]),
                                         AR.V(d9), AR.V(db))
        ref.append(p + v + q + AR.V(s[10:16]) + dbg + dba)
        orc.append(TDA._state_of(O.navstate_inc(TDA._navstate(s), d9, db)))
    return Table("ns_inc_unit", [c[0] for c in nc], ref, orc, TDA.STATE_PARTS)


@pytest.mark.gpu
def test_retraction_on_the_device():
    """ns_inc_unit by the rule and against ns_inc; ok from the program.  Applied 1000 times in a row the quaternion's
    norm stays within 4 ulp of 1: q_renorm takes out the first order of |q|^2 - 1 at every step, so what a step leaves
    is its own few roundings (and 3 / 8 e^2 of the e it met), not the sum of the steps before."""
    out, T, bad = device_outputs(), tables_N(), []
    nc = AC.vio_inc_cases()
    n = len(nc)
    assert {c[0].split("/")[0] for c in nc} >= {"dphi-norm=0", "dphi-norm=1e-9", "dphi-norm=0.49", "dphi-norm=0.51", "dphi-norm=3"}
    for k, c in enumerate(nc):
        if bool(out["N.ok"][k]) != c[4]:
            bad.append("ns_inc_unit/%s: ok is %d" % (c[0], out["N.ok"][k]))
    fast, plain, rep = out["N.ns_inc_unit"].reshape(n, 22), out["N.ns_inc"].reshape(n, 22), out["N.ns_inc_unit.repeated"].reshape(n, 22)
    bad += T.check_device(fast)
    bad += fast_vs_plain("ns_inc_unit q", [c[0] for c in nc], fast[:, 6:10], plain[:, 6:10], [r[6:10] for r in T.ref], T.bound,
                         [c[4] for c in nc])
    for what, a in (("once", fast), ("%d times" % REPS, rep)):
        n2 = [float(abs(sum(mpf(float(c)) ** 2 for c in r) - 1)) for r in a[:, 6:10]]
        k = int(np.argmax(n2))
        print("ns_inc_unit            %s: norm off by at most %.3g (%s)" % (what, n2[k] / 2, nc[k][0]))
        if not n2[k] / 2 <= 4 * EPS:
            bad.append("ns_inc_unit %s/%s: norm off by %.3g" % (what, nc[k][0], n2[k] / 2))
    assert np.isfinite(rep).all()
    assert not bad, "\n".join(bad[:60])


# ------------------------------------------------------------------ V. the visual edge
def test_float_values_need_no_excuse():
    """the as-written image points of the chosen cases lie further than EXCUSE_MARGIN from a float rounding boundary"""
    D = TDA.tables_D()
    assert min(D["margin"]) > EXCUSE_MARGIN, min(D["margin"])
    _, cams, _ = AC.cameras()
    assert all(int(cams[c[1]]["model"]) == 0 for c in AC.visual_cases())      # the frame's camera is a pinhole


@pytest.mark.gpu
def test_visual_edge_on_the_device():
    """A derived floor beside the rule on (chi2, err, Pc): with fused multiply-adds make_xf and Pc = Rcw Xw + tcw round
    otherwise than the oracle does, and at depth 0.3 m the stereo row's bf / z magnifies Pc's last bits by bf / z^2
    (three `Rcb=body` stereo cases came out at up to 36 x E_oracle; edge_error of ba_device.h, compiled here, gives the
    same bytes as vis_error_flat).  The floor is the ceiling tests/test_device_algebra.py reasons for this chain in
    test_visual_edge_reference_against_oracle: Pc cancels terms of size S down to the depth, 16 u S / |Pc|, and reaches
    the stereo residual through bf / z^2."""
    out, D, bad = device_outputs(), TDA.tables_D(), []
    tab, slots = AC.vio_visual_cases()
    vc = AC.visual_cases()
    nv, n = len(vc), len(slots)
    E, hub = out["V.vis_error_flat"].reshape(n, 9), out["V.edge_huber_flat"].reshape(n, 2)
    J, acc = out["V.vis_jacobian_flat"].reshape(n, 18), out["V.vis_accumulate_flat"].reshape(n, 27)
    valid = np.array([s[4] for s in slots], bool)
    te, tj = D["edge_eval<false>"], D["edge_eval<false>.J"]
    flat = np.hstack([E[:, 7:8], E[:, 0:3], E[:, 3:6]])           # chi2, err, Pc: the order of the table
    if not (E[:nv, 8] == np.array(D["stereo"], float)).all():
        bad.append("vis_error_flat: stereo flag")
    if not (E[:nv, 6] == np.array([c[4][6] for c in vc])).all():
        bad.append("vis_error_flat: info")
    # the float-rounded image point: u = o.u - err[0] exactly, so err[0..1] are the floats' differences, bit for bit
    excused = 0
    for k in range(nv):
        for j in range(2):
            if float(te.ref[k][1 + j]) != E[k, j]:
                if D["margin"][k] <= EXCUSE_MARGIN:
                    excused += 1
                else:
                    bad.append("vis_error_flat/%s: err[%d] is %r, as written %r" % (vc[k][0], j, E[k, j], float(te.ref[k][1 + j])))
    print("vis_error_flat         %d of %d float values excused" % (excused, 2 * nv))
    if excused > EXCUSE_CAP * 2 * nv:
        bad.append("vis_error_flat: %d values excused" % excused)
    def S(k):
        return 3 * (np.abs(vc[k][4][0:3]).max() + np.abs(vc[k][3][0:3]).max() + 1)

    def edge_floor(k, pi):
        Pc, err, z = (float(max(abs(x) for x in te.ref[k][a:b])) for a, b in ((4, 7), (1, 4), (6, 7)))
        e_err = (4 * U * 800 + 50 * 16 * U * S(k) / (z * z)) / err if err else 4 * U * 800
        return max(16 * U * S(k) / Pc, e_err, 2 * e_err + 8 * U)
    b, k_exc = TDA._excusing(check_floor(te, flat[:nv], edge_floor, indexed=True), D["margin"])
    bad += b
    worst = 0.0
    for k, name in enumerate(tj.names):
        e = rel_err(J[k, :18 if D["stereo"][k] else 12], tj.ref[k])
        worst = max(worst, e / tj.bound(k))
        if not e <= tj.bound(k):
            bad.append("vis_jacobian_flat/%s: error %.3g, bound %.3g" % (name, e, tj.bound(k)))
        if not D["stereo"][k] and J[k, 12:].any():
            bad.append("vis_jacobian_flat/%s: the stereo row of a monocular edge is not zero" % name)
    print("%-22s device worst ratio to its bound %.3f over %d cases" % ("vis_jacobian_flat", worst, nv))
    # fast against plain: the same operations in the same order -- within the two bounds (bytes, as a rule)
    pe, pj = out["V.edge_error"].reshape(n, 7), out["V.visual_jacobian"].reshape(n, 18)
    bad += fast_vs_plain("vis_error_flat", te.names, flat[:nv], pe[:nv], te.ref, te.bound, [True] * nv, TDA.EDGE_PARTS)
    same = int((bits(flat[:nv]) == bits(pe[:nv])).all(1).sum())
    print("vis_error_flat         %d of %d slots bit-equal to edge_error" % (same, nv))
    worst_h = worst_a = 0.0
    for k, s in enumerate(slots):
        if not s[4]:
            continue
        d, r = float(s[6]), s[8]
        ref, _ = AR.huber_aw(mpf(float(E[k, 7])), mpf(d), mpf(d * d))
        if not s[5]:
            if not (hub[k, 0] == E[k, 7] and hub[k, 1] == 1.0):
                bad.append("huber_flat/%s: robust = false must hand back (chi2, 1)" % s[0])
            ref = [mpf(float(E[k, 7])), mpf(1)]
        worst_h = max(worst_h, max(rel_err(hub[k, 0:1], ref[0:1]), rel_err(hub[k, 1:2], ref[1:2])) / (4 * EPS))
        Jk, err, info, r1, st = J[k], E[k, 0:3], float(s[3][6]), float(hub[k, 1]), D["stereo"][r]
        ra = AR.accumulate_aw(AR.V(Jk), AR.V(err), mpf(info), mpf(r1), st)
        w, rows = r1 * info, 3 if st else 2
        fa = [sum(Jk[q * 6 + a] * w * Jk[q * 6 + b] for q in range(rows)) for a in range(6) for b in range(a, 6)]
        fa += [sum(Jk[q * 6 + a] * (-(info * err[q]) * r1) for q in range(rows)) for a in range(6)]
        e_or = max(rel_err(fa[:21], ra[:21]), rel_err(fa[21:], ra[21:]))
        e = max(rel_err(acc[k, :21], ra[:21]), rel_err(acc[k, 21:], ra[21:]))
        worst_a = max(worst_a, e / (4 * max(e_or, EPS)))
        if not e <= 4 * max(e_or, EPS):
            bad.append("vis_accumulate_flat/%s: error %.3g, bound %.3g" % (s[0], e, 4 * max(e_or, EPS)))
    if not worst_h <= 1:
        bad.append("huber_flat at the edges' chi2: worst ratio %.3g" % worst_h)
    print("huber_flat (edge chi2) device worst ratio to its bound %.3f" % worst_h)
    print("vis_accumulate_flat    device worst ratio to its bound %.3f" % worst_a)
    # slots that do not count: the sums keep their bytes, everything is finite
    masked = np.flatnonzero(~valid)
    assert len(masked) == 6
    acc0 = np.array([s[7] for s in slots])
    for k in masked:
        if not (bits(acc[k]) == bits(acc0[k])).all():
            bad.append("vis_accumulate_flat/%s: weight 0 changed the sums" % slots[k][0])
        if not (np.isfinite(E[k]).all() and np.isfinite(hub[k]).all() and np.isfinite(J[k]).all() and np.isfinite(acc[k]).all()):
            bad.append("%s: a value is not finite" % slots[k][0])
    # huber_flat on the named widths: the rule, and the branch as far as the outputs show it
    hc = AC.vio_huber_cases()
    hf, hp = out["V.huber_flat"].reshape(-1, 2), out["V.huber"].reshape(-1, 2)
    TH, nh = D["huber"], len(AC.huber_cases())
    bad += TH.check_device(hf[:nh])
    for k, c in enumerate(hc):
        j = k if k < nh else k - nh
        quad = D["huber.branch"][j] == "quadratic" or not c[4]
        if quad and not (hf[k, 0] == c[1] and hf[k, 1] == 1.0):
            bad.append("huber_flat/%s: not (e, 1)" % c[0])
        if not quad and 1 - TH.ref[j][1] > 4 * EPS and not hf[k, 1] < 1.0:
            bad.append("huber_flat/%s: not the linear branch" % c[0])
        if c[4] and not (bits(hf[k]) == bits(hp[k])).all():
            bad.append("huber_flat/%s: not huber's bytes" % c[0])
    hn = [c[0] for c in hc]
    for w in ("mono", "stereo", "encoder"):
        assert {"%s/e=dsqr" % w, "%s/e-below-dsqr" % w, "%s/e-above-dsqr" % w} <= set(hn)
    assert not bad, "\n".join(bad[:60])


# ------------------------------------------------------------------ S. the solver
def _shifted(H, lam):
    A = np.array(H, np.float64).copy()
    A[np.diag_indices_from(A)] += lam
    return A


def rho(H, lam, b, x):
    """the scaled componentwise residual max_i |b - (H + lam I) x|_i / (sum_j sqrt(a_ii a_jj) |x_j| + |b_i|), x taken
    into 50 digits"""
    n = len(b)
    A = [[mpf(float(H[i][j])) + (mpf(float(lam)) if i == j else 0) for j in range(n)] for i in range(n)]
    xs = AR.V(x)
    worst = mpf(0)
    for i in range(n):
        r = abs(mpf(float(b[i])) - sum(A[i][j] * xs[j] for j in range(n)))
        s = sum(mpmath.sqrt(A[i][i] * A[j][j]) * abs(xs[j]) for j in range(n)) + abs(mpf(float(b[i])))
        worst = max(worst, r / s)
    return float(worst)


def test_solver_cases_have_the_stated_structure():
    sc = AC.vio_solver_cases()
    assert {c[1] for c in sc} == {15, 30} and len(sc) <= 64
    for name, n, H, b, lam, solvable in sc:
        H = np.asarray(H)
        for t in range(6):
            row = H[9 + t].copy()
            row[9 + t] = 0
            if n == 30:
                row[24 + t] = 0
            assert not row.any() and not np.nan_to_num(H[:, 9 + t] - H[9 + t]).any(), name
        if solvable:
            A = _shifted(H, lam)
            assert (A == A.T).all() and np.linalg.eigvalsh(A).min() > 0, name
            if "cond-1e2" in name:
                assert 30 < np.linalg.cond(A) < 1e3, (name, np.linalg.cond(A))
            if "vio-scaled" in name:
                d = np.sqrt(np.diag(A))
                assert d.max() / d.min() > 1e5, name
            if "coupling" in name:
                for t in range(6):
                    assert 0 < 1 - abs(A[9 + t, 24 + t]) / math.sqrt(A[9 + t, 9 + t] * A[24 + t, 24 + t]) < 1e-6
        elif "middle-pivot" in name:
            assert (np.diag(H) > 0).all() and np.linalg.eigvalsh(H).min() < 0
        else:
            assert not (np.diag(H) > 0).all(), name
    lams = {c[0].split("lambda=")[1] for c in sc if "lambda=" in c[0]}
    assert lams == {"0", "1e-8-mean-diagonal", "smallest-diagonal", "10-largest-diagonal"}
    assert sc[-1][0].endswith("again-in-the-last-workgroup") and sc[-1][2] is sc[0][2]


@pytest.mark.gpu
def test_solver_on_the_device():
    out, bad = device_outputs(), []
    sc = AC.vio_solver_cases()
    inp = program_inputs()
    X, ret = out["S.x"].reshape(len(sc), 32), out["S.ok"]
    worst_r = worst_f = 0.0
    for k, (name, n, H, b, lam, solvable) in enumerate(sc):
        if not solvable:
            if ret[k] != 0:
                bad.append("%s: returned true" % name)
            if not (bits(X[k]) == bits(inp["S.x0"][k])).all():
                bad.append("%s: x changed although the solve failed" % name)
            continue
        if ret[k] != 1:
            bad.append("%s: returned false" % name)
            continue
        if not (bits(X[k, n:]) == bits(inp["S.x0"][k, n:])).all():
            bad.append("%s: wrote beyond x[n]" % name)
        A = _shifted(H, lam)
        xl = np.linalg.solve(A, b)
        r_dev, r_lap = rho(H, lam, b, X[k, :n]), rho(H, lam, b, xl)
        lim = 4 * max(r_lap, n * EPS)
        worst_r = max(worst_r, r_dev / lim)
        line = "%-44s rho device %.3g, numpy %.3g" % (name, r_dev, r_lap)
        if not r_dev <= lim:
            bad.append("%s: rho %.3g, limit %.3g (numpy %.3g)" % (name, r_dev, lim, r_lap))
        cond = float(np.linalg.cond(A))
        if cond < 1e3:
            xr = AR.solve_shifted_ex(H, lam, b)
            e_dev, e_lap = rel_err(X[k, :n], xr), rel_err(xl, xr)
            lim = 4 * max(e_lap, n * EPS)
            worst_f = max(worst_f, e_dev / lim)
            line += "; forward error device %.3g, numpy %.3g (cond %.3g)" % (e_dev, e_lap, cond)
            if not e_dev <= lim:
                bad.append("%s: forward error %.3g, limit %.3g (E_lapack %.3g, cond %.3g)" % (name, e_dev, lim, e_lap, cond))
        print(line)
    print("wave_solve_vio         worst ratio to its limit: rho %.3f, forward error %.3f" % (worst_r, worst_f))
    if not (bits(X[0, :sc[0][1]]) == bits(X[-1, :sc[0][1]])).all():
        bad.append("the same case in the first and the last workgroup: different bytes")
    assert not bad, "\n".join(bad[:60])


def test_program_cross_compiles_for_gfx950():
    """drift of the header against the program is caught without a GPU; the library's flags, no warning"""
    exe, log = built_program()
    assert exe is not None, log
    assert os.path.getsize(exe) > 0 and "warning" not in log, log


def test_case_lists_stay_small():
    inp = program_inputs()
    assert max(len(inp[k]) for k in ("R.rotvec", "R.quat", "P.prior", "I.meas", "N.state", "V.cam", "V.huber_e")) <= 512
    assert sum(a.nbytes for a in inp.values()) < 2 << 20
