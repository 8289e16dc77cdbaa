"""IMUPreIntegratorBase::PreIntegration + update (reference src/Odom/OdomPreIntegrator.h:226-506):
oracle known-answer tests against the numpy restatement of update() in synth_ba (CPU) and HIP-vs-oracle parity."""
import numpy as np
import pytest

from vieo_slam_amd import synth_ba
from vieo_slam_amd.ba_types import IMU_PREINT_DTYPE
from vieo_slam_amd.imu import IMU_NOISE_DTYPE, IMU_SAMPLE_DTYPE


def _noise(fixed=1):
    N = np.zeros(1, IMU_NOISE_DTYPE)
    f = synth_ba.IMU_FREQ if fixed else 1.0
    N[0]["sigma_g"] = (np.eye(3) * synth_ba.IMU_SIGMA[0] ** 2 * f).reshape(-1)
    N[0]["sigma_a"] = (np.eye(3) * synth_ba.IMU_SIGMA[1] ** 2 * f).reshape(-1)
    N[0]["freq_ref"], N[0]["dt_cov_noise_fixed"] = synth_ba.IMU_FREQ, fixed
    return N


def _samples(rng, t0, n, h=0.005, jitter=0.0):
    s = np.zeros(n, IMU_SAMPLE_DTYPE)
    s["t"] = t0 + np.arange(n) * h + rng.uniform(-jitter, jitter, n)
    s["w"] = rng.normal(0, 0.4, (1, 3)) + rng.normal(0, 0.05, (n, 3))
    s["a"] = rng.normal(0, 2.0, (1, 3)) + np.array([0, 0, 9.8]) + rng.normal(0, 0.2, (n, 3))
    return s


def test_oracle_matches_numpy_update_on_aligned_samples(oracle):
    rng = np.random.default_rng(1)
    s = _samples(rng, 10.0, 21)
    bg, ba = rng.normal(0, 0.01, 3), rng.normal(0, 0.05, 3)
    out, prv, st = oracle.imu_preintegrate(_noise(), [s], [s["t"][0]], [s["t"][-1]], [bg], [ba])
    P = synth_ba.Preintegrator()
    for k in range(20):
        P.update((s["w"][k] + s["w"][k + 1]) / 2 - bg, (s["a"][k] + s["a"][k + 1]) / 2 - ba, s["t"][k + 1] - s["t"][k])
    o = out[0]
    assert st[0] == 0 and abs(o["dt"] - 0.1) < 1e-12
    assert np.allclose(o["Rij"].reshape(3, 3), P.R, atol=1e-13) and np.allclose(o["vij"], P.v, atol=1e-13)
    assert np.allclose(o["pij"], P.p, atol=1e-14)
    for k, ref in (("JgR", P.JgR), ("Jgv", P.Jgv), ("Jav", P.Jav), ("Jgp", P.Jgp), ("Jap", P.Jap)):
        assert np.allclose(o[k].reshape(3, 3), ref, atol=1e-13), k
    S = o["Sigma"].reshape(9, 9)
    assert np.allclose(S, P.Sigma, rtol=1e-10, atol=1e-20)
    # mSigmaijPRV is the same covariance with the v and Phi blocks exchanged
    perm = [0, 1, 2, 6, 7, 8, 3, 4, 5]
    assert np.allclose(prv[0], S[np.ix_(perm, perm)], rtol=1e-10, atol=1e-20)
    assert np.allclose(S, S.T, rtol=1e-9) and np.linalg.eigvalsh(S).min() > 0


def test_oracle_partial_intervals_and_status(oracle):
    rng = np.random.default_rng(2)
    s = _samples(rng, 5.0, 30)
    s["w"], s["a"] = s["w"][0], s["a"][0]  # constant measurements: interpolation cannot change them
    bg = ba = np.zeros(3)
    ti, tj = s["t"][3] + 0.002, s["t"][24] + 0.001  # both ends inside a sample interval
    out, prv, st = oracle.imu_preintegrate(_noise(), [s], [ti], [tj], [bg], [ba])
    assert st[0] == 0 and abs(out[0]["dt"] - (tj - ti)) < 1e-12
    # constant rate: R = Exp(w * T) whatever the splitting
    assert np.allclose(out[0]["Rij"].reshape(3, 3), synth_ba.so3_exp(s["w"][0] * (tj - ti)), atol=1e-12)
    # the window may start before the first and end after the last sample
    out2, _, st2 = oracle.imu_preintegrate(_noise(), [s[5:15]], [s["t"][5] - 0.003], [s["t"][14] + 0.004], [bg], [ba])
    assert st2[0] == 0 and abs(out2[0]["dt"] - (s["t"][14] + 0.004 - s["t"][5] + 0.003)) < 1e-12
    # statuses: no samples / a 2 s hole
    hole = s.copy()
    hole["t"][15:] += 2.0
    _, _, st3 = oracle.imu_preintegrate(_noise(), [s[:0], hole], [5.0, hole["t"][0]], [5.1, hole["t"][-1]], [bg] * 2,
                                        [ba] * 2)
    assert st3.tolist() == [1, 2]
    # noise model: per-sample 1/dt scaling equals the fixed one at the reference rate
    a, _, _ = oracle.imu_preintegrate(_noise(1), [s], [s["t"][0]], [s["t"][-1]], [bg], [ba])
    b, _, _ = oracle.imu_preintegrate(_noise(0), [s], [s["t"][0]], [s["t"][-1]], [bg], [ba])
    assert np.allclose(a[0]["Sigma"], b[0]["Sigma"], rtol=1e-6)


def test_oracle_backward_order(oracle):
    """timeStampi > timeStampj (map reuse, OdomPreIntegrator.h:241-262): the samples are walked backwards with
    negative steps.  Constant measurements have closed forms whatever the splitting: R = Exp(w T), and with w = 0
    v = a T, p = a T^2 / 2 (T = tj - ti < 0); the forward run over the same span mirrors them."""
    rng = np.random.default_rng(4)
    s = _samples(rng, 5.0, 30)
    bg = ba = np.zeros(3)
    for ti, tj in ((s["t"][24] + 0.001, s["t"][3] + 0.002),   # both ends inside a sample interval
                   (s["t"][29] + 0.004, s["t"][0] - 0.003),   # beyond both ends of the list
                   (s["t"][20], s["t"][5]),                   # on samples
                   (s["t"][7] + 0.0031, s["t"][7] + 0.0012)):  # inside one interval
        c = s.copy()
        c["w"], c["a"] = s["w"][0], 0.0
        out, _, st = oracle.imu_preintegrate(_noise(), [c], [ti], [tj], [bg], [ba])
        T = tj - ti
        assert st[0] == 0 and T < 0 and abs(out[0]["dt"] - T) < 1e-12, (ti, tj, out[0]["dt"])
        assert np.allclose(out[0]["Rij"].reshape(3, 3), synth_ba.so3_exp(s["w"][0] * T), atol=1e-12)
        c["w"], c["a"] = 0.0, s["a"][0]
        out, _, st = oracle.imu_preintegrate(_noise(), [c], [ti], [tj], [bg], [ba])
        assert np.allclose(out[0]["vij"], s["a"][0] * T, atol=1e-12) and np.allclose(out[0]["pij"], s["a"][0] * T * T / 2, atol=1e-12)
    # varying measurements: forward over [a, b] then backward over [b, a] compose to (nearly) the identity rotation
    a, b = s["t"][2] + 0.001, s["t"][26] + 0.003
    f, _, _ = oracle.imu_preintegrate(_noise(), [s], [a], [b], [bg], [ba])
    r, _, st = oracle.imu_preintegrate(_noise(), [s], [b], [a], [bg], [ba])
    assert st[0] == 0 and abs(f[0]["dt"] + r[0]["dt"]) < 1e-12
    assert np.abs(f[0]["Rij"].reshape(3, 3) @ r[0]["Rij"].reshape(3, 3) - np.eye(3)).max() < 1e-5
    # a hole is still refused
    hole = s.copy()
    hole["t"][15:] += 2.0
    _, _, st = oracle.imu_preintegrate(_noise(), [hole], [hole["t"][-1]], [hole["t"][0]], [bg], [ba])
    assert st[0] == 2


@pytest.mark.gpu
def test_preintegration_parity(oracle):
    from vieo_slam_amd.imu import imu_preintegrate
    rng = np.random.default_rng(3)
    lists, ti, tj = [], [], []
    for k in range(700):
        n = int(rng.integers(0, 40)) if k else 0
        s = _samples(rng, 100.0 + k, n, jitter=0.001)
        if n > 3 and k % 50 == 7:
            s["t"][n // 2:] += 2.0
        lists.append(s)
        if n:
            ti.append(s["t"][0] + rng.uniform(-0.004, 0.012))
            tj.append(s["t"][-1] + rng.uniform(-0.012, 0.004))
            if k % 3 == 2:  # backward order (map reuse)
                ti[-1], tj[-1] = tj[-1], ti[-1]
        else:
            ti.append(0.0), tj.append(1.0)
    bg, ba = rng.normal(0, 0.01, (700, 3)), rng.normal(0, 0.05, (700, 3))
    for fixed in (1, 0):
        o, op, os_ = oracle.imu_preintegrate(_noise(fixed), lists, ti, tj, bg, ba)
        h, hp, hs = imu_preintegrate(_noise(fixed), lists, ti, tj, bg, ba)
        assert np.array_equal(os_, hs) and set(os_.tolist()) >= {0, 1, 2}
        for k in ("dt", "Rij", "vij", "pij", "JgR", "Jgv", "Jav", "Jgp", "Jap"):
            assert np.allclose(o[k], h[k], rtol=1e-11, atol=1e-13), k
        # covariances: relative to each matrix's own scale (tiny off-diagonal entries are differences of products)
        for a, b in ((o["Sigma"], h["Sigma"]), (op.reshape(700, 81), hp.reshape(700, 81))):
            # (a zero-length sub-step with the 1/dt noise model gives inf * 0 = NaN in the reference as well)
            assert np.array_equal(np.isnan(a), np.isnan(b))
            a, b = np.nan_to_num(a), np.nan_to_num(b)
            scale = np.abs(a).max(1, keepdims=True) + 1e-300
            assert (np.abs(a - b) / scale).max() < 1e-10


@pytest.mark.gpu
def test_wave_and_lane_instantiations_agree_bitwise():
    """A call with fewer than 1024 intervals gives every interval a wavefront (the 9 x 9 products spread over the lanes),
    a larger one a lane: every entry is summed by one lane in the same order, so the two must agree bit for bit."""
    from vieo_slam_amd.imu import imu_preintegrate
    rng = np.random.default_rng(11)
    lists, ti, tj = [], [], []
    for k in range(1100):
        n = int(rng.integers(2, 120))
        s = _samples(rng, 50.0 + k, n, jitter=0.001)
        lists.append(s)
        ti.append(s["t"][0] + rng.uniform(-0.004, 0.012))
        tj.append(s["t"][-1] + rng.uniform(-0.012, 0.004))
        if k % 4 == 3:
            ti[-1], tj[-1] = tj[-1], ti[-1]
    bg, ba = rng.normal(0, 0.01, (1100, 3)), rng.normal(0, 0.05, (1100, 3))
    for fixed in (1, 0):
        big, bigp, bigs = imu_preintegrate(_noise(fixed), lists, ti, tj, bg, ba)               # lane per interval
        sm, smp, sms = imu_preintegrate(_noise(fixed), lists[:40], ti[:40], tj[:40], bg[:40], ba[:40])  # wavefront each
        assert np.array_equal(bigs[:40], sms)
        assert big[:40].tobytes() == sm.tobytes()
        assert np.asarray(bigp)[:40].tobytes() == np.asarray(smp).tobytes()


# ---------------------------------------------------------------- continuation (breset = false) ----------------
# PreIntegration(..., breset = false) skips reset() and runs update() on from the members (OdomPreIntegrator.h:232-234):
# Tracking::PreIntegration passes it for every frame after the first one behind a key frame (include/Tracking.h:417).

_MEMBERS = ("dt", "Rij", "vij", "pij", "JgR", "Jgv", "Jav", "Jgp", "Jap", "Sigma")


def _reset_seed(n):
    s = np.zeros(n, IMU_PREINT_DTYPE)
    s["Rij"] = np.eye(3).reshape(-1)
    return s, np.zeros((n, 9, 9))


def _chain(run, lists, times, bg, ba, seed=None, seed_prv=None):
    """PreIntegration over [times[0], times[1]], then continued over [times[i - 1], times[i]] (one list per call):
    the outputs of every call"""
    outs = []
    for i in range(1, len(times)):
        cont = seed is not None or i > 1
        o, p, st = run(lists[i - 1], times[i - 1], times[i], bg, ba, seed, seed_prv, 0 if cont else 1)
        outs.append((o, p, st))
        seed, seed_prv = o, p
    return outs


def _oracle_run(oracle, fixed=1):
    def run(s, ti, tj, bg, ba, seed, seed_prv, breset):
        if seed is None:
            seed, seed_prv = _reset_seed(1)
        return oracle.imu_preintegrate(_noise(fixed), [s], [ti], [tj], [bg], [ba], seed, seed_prv, [breset])
    return run


def _sub(s, t0, t1):
    """the samples the reference hands over for [t0, t1] (Tracking.h:399-428: from the last one at or before the
    earlier time to the first one at or after the later)"""
    lo, hi = min(t0, t1), max(t0, t1)
    i0 = max(int(np.searchsorted(s["t"], lo, "right")) - 1, 0)
    i1 = min(int(np.searchsorted(s["t"], hi, "left")) + 1, len(s))
    return s[i0:i1]


def test_oracle_continuation_matches_numpy(oracle):
    """a reset call over [t_0, t_10], continued over [t_10, t_24] with another bias: synth_ba.Preintegrator run on
    without a reset"""
    rng = np.random.default_rng(21)
    s = _samples(rng, 10.0, 25)
    bg1, ba1 = rng.normal(0, 0.01, 3), rng.normal(0, 0.05, 3)
    bg2, ba2 = rng.normal(0, 0.01, 3), rng.normal(0, 0.05, 3)
    a, ap, st = oracle.imu_preintegrate(_noise(), [s], [s["t"][0]], [s["t"][10]], [bg1], [ba1])
    o, prv, st2 = oracle.imu_preintegrate(_noise(), [s], [s["t"][10]], [s["t"][24]], [bg2], [ba2], a, ap, [0])
    P = synth_ba.Preintegrator()
    for k in range(24):
        bg, ba = (bg1, ba1) if k < 10 else (bg2, ba2)
        P.update((s["w"][k] + s["w"][k + 1]) / 2 - bg, (s["a"][k] + s["a"][k + 1]) / 2 - ba, s["t"][k + 1] - s["t"][k])
    o = o[0]
    assert st[0] == st2[0] == 0 and abs(o["dt"] - (s["t"][24] - s["t"][0])) < 1e-12
    assert np.allclose(o["Rij"].reshape(3, 3), P.R, atol=1e-13) and np.allclose(o["vij"], P.v, atol=1e-13)
    assert np.allclose(o["pij"], P.p, atol=1e-14)
    for k, ref in (("JgR", P.JgR), ("Jgv", P.Jgv), ("Jav", P.Jav), ("Jgp", P.Jgp), ("Jap", P.Jap)):
        assert np.allclose(o[k].reshape(3, 3), ref, atol=1e-13), k
    S = o["Sigma"].reshape(9, 9)
    assert np.allclose(S, P.Sigma, rtol=1e-10, atol=1e-20)
    perm = [0, 1, 2, 6, 7, 8, 3, 4, 5]
    assert np.allclose(prv[0], S[np.ix_(perm, perm)], rtol=1e-10, atol=1e-20)
    # the continuation really started from the seed: a reset call over the second span alone is far from it
    b, _, _ = oracle.imu_preintegrate(_noise(), [s], [s["t"][10]], [s["t"][24]], [bg2], [ba2])
    assert not np.allclose(b[0]["Rij"].reshape(3, 3), P.R, atol=1e-6)


def test_oracle_reset_seed_continues_like_a_reset(oracle):
    rng = np.random.default_rng(22)
    s = _samples(rng, 3.0, 40, jitter=0.001)
    bg, ba = rng.normal(0, 0.01, 3), rng.normal(0, 0.05, 3)
    for fixed in (1, 0):
        for ti, tj in ((s["t"][0] + 0.002, s["t"][-1] - 0.001), (s["t"][30] + 0.001, s["t"][4] + 0.003)):
            seed, seed_prv = _reset_seed(1)
            a = oracle.imu_preintegrate(_noise(fixed), [s], [ti], [tj], [bg], [ba])
            b = oracle.imu_preintegrate(_noise(fixed), [s], [ti], [tj], [bg], [ba], seed, seed_prv, [0])
            c = oracle.imu_preintegrate(_noise(fixed), [s], [ti], [tj], [bg], [ba], seed, seed_prv, [1])
            for x, y, z in zip(a, b, c):
                assert x.tobytes() == y.tobytes() == z.tobytes()


@pytest.mark.parametrize("sub", [False, True])
def test_oracle_chained_at_sample_times_equals_one_call(oracle, sub):
    """each continuation starts at the previous end, snapped to a sample time (Tracking.h:411-416 cur_time2): the
    chain makes the same update() calls as one call over the whole span, forward and backward (map reuse).
    sub: every call gets the reference's sub-list around its span, else the whole list"""
    rng = np.random.default_rng(23)
    s = _samples(rng, 7.0, 60, jitter=0.001)
    bg, ba = rng.normal(0, 0.01, 3), rng.normal(0, 0.05, 3)
    t = s["t"]
    fwd = [t[2] + 0.0013, t[9], t[10], t[23], t[41], t[58] + 0.0021]
    back = [t[57] + 0.0017, t[40], t[22], t[21], t[6], t[3] + 0.0009]  # (never split at the first sample: :254-259)
    for fixed in (1, 0):
        run = _oracle_run(oracle, fixed)
        for times in (fwd, back):
            lists = [_sub(s, times[i], times[i + 1]) if sub else s for i in range(len(times) - 1)]
            chain = _chain(run, lists, times, bg, ba)
            one = oracle.imu_preintegrate(_noise(fixed), [s], [times[0]], [times[-1]], [bg], [ba])
            assert [c[2][0] for c in chain] == [0] * (len(times) - 1)
            for x, y in zip(chain[-1], one):
                assert x.tobytes() == y.tobytes()


def test_oracle_empty_continuation_returns_the_seed(oracle):
    rng = np.random.default_rng(24)
    s = _samples(rng, 1.0, 30)
    bg, ba = rng.normal(0, 0.01, 3), rng.normal(0, 0.05, 3)
    seed, seed_prv, _ = oracle.imu_preintegrate(_noise(), [s], [s["t"][1] + 0.001], [s["t"][28]], [bg], [ba])
    o, p, st = oracle.imu_preintegrate(_noise(), [s[:0]], [s["t"][28]], [s["t"][29]], [bg], [ba], seed, seed_prv, [0])
    assert st[0] == 1 and o.tobytes() == seed.tobytes() and p.tobytes() == seed_prv.tobytes()
    # with breset the empty call still resets (outputs zeroed, dt = 0)
    o, p, st = oracle.imu_preintegrate(_noise(), [s[:0]], [s["t"][28]], [s["t"][29]], [bg], [ba], seed, seed_prv, [1])
    r, rp = _reset_seed(1)
    assert st[0] == 1 and o.tobytes() == r.tobytes() and p.tobytes() == rp.tobytes()


def test_oracle_gap_in_a_continuation(oracle):
    """a 2 s hole inside a continued span: mdeltatij = 0, -1 (:288-292), the other members as advanced up to the hole
    -- the same as a continuation that stops at the last sample before it"""
    rng = np.random.default_rng(25)
    s = _samples(rng, 20.0, 50)
    s["t"][30:] += 2.0
    bg, ba = rng.normal(0, 0.01, 3), rng.normal(0, 0.05, 3)
    seed, seed_prv, _ = oracle.imu_preintegrate(_noise(), [s], [s["t"][2] + 0.001], [s["t"][12]], [bg], [ba])
    for fixed in (1, 0):
        g, gp, gs = oracle.imu_preintegrate(_noise(fixed), [s], [s["t"][12]], [s["t"][40] + 0.002], [bg], [ba], seed,
                                            seed_prv, [0])
        h, hp, hs = oracle.imu_preintegrate(_noise(fixed), [s], [s["t"][12]], [s["t"][29]], [bg], [ba], seed,
                                            seed_prv, [0])
        assert gs[0] == 2 and hs[0] == 0 and g[0]["dt"] == 0 and h[0]["dt"] > seed[0]["dt"] > 0
        for k in _MEMBERS[1:]:
            assert g[0][k].tobytes() == h[0][k].tobytes(), k
        assert gp.tobytes() == hp.tobytes()
        # backward over the hole: the same rule
        b, bp, bs = oracle.imu_preintegrate(_noise(fixed), [s], [s["t"][40]], [s["t"][12]], [bg], [ba], seed,
                                            seed_prv, [0])
        c, cp, cs = oracle.imu_preintegrate(_noise(fixed), [s], [s["t"][40]], [s["t"][30]], [bg], [ba], seed,
                                            seed_prv, [0])
        assert bs[0] == 2 and cs[0] == 0 and b[0]["dt"] == 0
        for k in _MEMBERS[1:]:
            assert b[0][k].tobytes() == c[0][k].tobytes(), k


def _seeded_batch(rng, n, seeds, seeds_prv, t0=200.0):
    """n intervals that mix reset and continue, forward and backward, empty lists and 2 s holes; seed k is an earlier
    output (seeds[j] for a random j), its bias changed for every other continued interval"""
    lists, ti, tj = [], [], []
    for k in range(n):
        m = int(rng.integers(0, 40)) if k % 23 else 0
        s = _samples(rng, t0 + k, m, jitter=0.001)
        if m > 3 and k % 50 == 7:
            s["t"][m // 2:] += 2.0
        lists.append(s)
        if m:
            ti.append(s["t"][0] + rng.uniform(-0.004, 0.012))
            tj.append(s["t"][-1] + rng.uniform(-0.012, 0.004))
            if k % 3 == 2:
                ti[-1], tj[-1] = tj[-1], ti[-1]
        else:
            ti.append(t0 + k), tj.append(t0 + k + 0.05)
    j = rng.integers(0, len(seeds), n)
    seed, seed_prv = seeds[j].copy(), seeds_prv[j].copy()
    breset = (np.arange(n) % 5 == 1).astype(np.int32)
    return lists, ti, tj, seed, seed_prv, breset


def _first_batch(oracle, rng, fixed, n=300):
    lists = [_samples(rng, 100.0 + k, int(rng.integers(2, 40)), jitter=0.001) for k in range(n)]
    ti = [s["t"][0] + rng.uniform(-0.004, 0.012) for s in lists]
    tj = [s["t"][-1] + rng.uniform(-0.012, 0.004) for s in lists]
    bg, ba = rng.normal(0, 0.01, (n, 3)), rng.normal(0, 0.05, (n, 3))
    o, op, _ = oracle.imu_preintegrate(_noise(fixed), lists, ti, tj, bg, ba)
    return o, op, bg, ba


@pytest.mark.gpu
def test_continuation_parity(oracle):
    """~700 intervals in one call, seeded from earlier outputs: the kernel against the oracle to the tolerances of
    test_preintegration_parity; an empty continued list returns its seed"""
    from vieo_slam_amd.imu import imu_preintegrate
    rng = np.random.default_rng(41)
    n = 700
    for fixed in (1, 0):
        seeds, seeds_prv, bg0, ba0 = _first_batch(oracle, rng, fixed)
        lists, ti, tj, seed, seed_prv, breset = _seeded_batch(rng, n, seeds, seeds_prv)
        bg, ba = rng.normal(0, 0.01, (n, 3)), rng.normal(0, 0.05, (n, 3))
        same = np.arange(n) % 2 == 0  # every other interval continues with the bias of its seed's call
        j = rng.integers(0, len(bg0), n)
        bg[same], ba[same] = bg0[j[same]], ba0[j[same]]
        o, op, os_ = oracle.imu_preintegrate(_noise(fixed), lists, ti, tj, bg, ba, seed, seed_prv, breset)
        h, hp, hs = imu_preintegrate(_noise(fixed), lists, ti, tj, bg, ba, seed, seed_prv, breset)
        assert np.array_equal(os_, hs) and set(os_.tolist()) >= {0, 1, 2}
        cont = breset == 0
        assert (cont & (hs == 1)).any() and (cont & (hs == 2)).any() and (~cont & (hs == 1)).any()
        for k in _MEMBERS[:-1]:
            assert np.allclose(o[k], h[k], rtol=1e-11, atol=1e-13), k
        for a, b in ((o["Sigma"], h["Sigma"]), (op.reshape(n, 81), hp.reshape(n, 81))):
            assert np.array_equal(np.isnan(a), np.isnan(b))
            a, b = np.nan_to_num(a), np.nan_to_num(b)
            scale = np.abs(a).max(1, keepdims=True) + 1e-300
            assert (np.abs(a - b) / scale).max() < 1e-10
        e = cont & (hs == 1)
        assert h[e].tobytes() == seed[e].tobytes() and hp[e].tobytes() == seed_prv[e].tobytes()
        g = cont & (hs == 2)
        assert (h["dt"][g] == 0).all()


def _chain_case(rng, k):
    """interval k's samples and the times of a chain split at sample times (backward for every third interval, never
    split at the first sample)"""
    m = int(rng.integers(12, 90))
    s = _samples(rng, 500.0 + k, m, jitter=0.001)
    cut = np.sort(rng.choice(np.arange(2, m - 2), 2, replace=False))
    times = [s["t"][0] + rng.uniform(-0.004, 0.004), s["t"][cut[0]], s["t"][cut[1]], s["t"][-1] + rng.uniform(-0.004, 0.004)]
    if k % 3 == 2:
        times = times[::-1]
    return s, times


@pytest.mark.gpu
@pytest.mark.parametrize("n", [40, 1100])
def test_chained_at_sample_times_equals_one_call_on_gpu(n):
    """n < 1024: a wavefront per interval, n >= 1024: a lane: in both, a chain of a reset call and two continuations
    split at sample times gives the bytes of one call over the whole span"""
    from vieo_slam_amd.imu import imu_preintegrate
    rng = np.random.default_rng(42)
    cases = [_chain_case(rng, k) for k in range(n)]
    lists = [c[0] for c in cases]
    bg, ba = rng.normal(0, 0.01, (n, 3)), rng.normal(0, 0.05, (n, 3))
    for fixed in (1, 0):
        seed = seed_prv = None
        for i in range(3):
            ti, tj = [c[1][i] for c in cases], [c[1][i + 1] for c in cases]
            breset = None if seed is None else np.zeros(n, np.int32)
            seed, seed_prv, st = imu_preintegrate(_noise(fixed), lists, ti, tj, bg, ba, seed, seed_prv, breset)
            assert (st == 0).all()
        one, onep, st = imu_preintegrate(_noise(fixed), lists, [c[1][0] for c in cases], [c[1][-1] for c in cases], bg, ba)
        assert (st == 0).all()
        assert seed.tobytes() == one.tobytes() and seed_prv.tobytes() == onep.tobytes()


@pytest.mark.gpu
def test_wave_and_lane_instantiations_agree_bitwise_with_seeds(oracle):
    from vieo_slam_amd.imu import imu_preintegrate
    rng = np.random.default_rng(43)
    n = 1100
    for fixed in (1, 0):
        seeds, seeds_prv, _, _ = _first_batch(oracle, rng, fixed)
        lists, ti, tj, seed, seed_prv, breset = _seeded_batch(rng, n, seeds, seeds_prv)
        bg, ba = rng.normal(0, 0.01, (n, 3)), rng.normal(0, 0.05, (n, 3))
        big, bigp, bigs = imu_preintegrate(_noise(fixed), lists, ti, tj, bg, ba, seed, seed_prv, breset)
        m = 200
        sm, smp, sms = imu_preintegrate(_noise(fixed), lists[:m], ti[:m], tj[:m], bg[:m], ba[:m], seed[:m],
                                        seed_prv[:m], breset[:m])
        assert set(sms.tolist()) >= {0, 1, 2}
        assert np.array_equal(bigs[:m], sms)
        assert big[:m].tobytes() == sm.tobytes() and bigp[:m].tobytes() == smp.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [300, 1100])
def test_old_entry_and_ex_entry_with_null_seed_agree(n):
    from vieo_slam_amd._lib import lib
    from vieo_slam_amd.imu import preint_call
    rng = np.random.default_rng(44)
    lists, ti, tj, _, _, _ = _seeded_batch(rng, n, *_reset_seed(1))
    bg, ba = rng.normal(0, 0.01, (n, 3)), rng.normal(0, 0.05, (n, 3))
    for fixed in (1, 0):
        a = preint_call(lib().vieo_imu_preintegrate_batch, _noise(fixed), lists, ti, tj, bg, ba)
        b = preint_call(lib().vieo_imu_preintegrate_batch_ex, _noise(fixed), lists, ti, tj, bg, ba, ex=True)
        assert a[0] == b[0] == 0
        for x, y in zip(a[1:], b[1:]):
            assert x.tobytes() == y.tobytes()
