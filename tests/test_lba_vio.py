"""LocalBundleAdjustmentNavStatePRV (a18): oracle known-answer tests (CPU) and GPU parity."""
import numpy as np
import pytest

from vieo_slam_amd import synth_ba
from vieo_slam_amd.ba_types import NAVSTATE_DTYPE


def _errs(navs, gt):
    n = gt["n_local"]
    dp = np.linalg.norm(navs["p"][:n] - gt["p"][:n], axis=1)
    dv = np.linalg.norm(navs["v"][:n] - gt["v"][:n], axis=1)
    dr = np.array([synth_ba.pose_error(navs[k], dict(p=navs[k]["p"], q=gt["q"][k]))[1] for k in range(n)])
    return dp, dr, dv


def test_oracle_prv_edge_jacobian_matches_central_differences(oracle):
    """EdgeNavStatePRV::linearizeOplus (g2otypes.h:777-884) against central differences of computeError
    through the vertices' own oplus (PR: p += R dp, R *= Exp(dphi); V, Bias additive)."""
    params, kfs, pts, close, obs, imu, gt = synth_ba.make_lba_vio_problem(3, n_local=3, n_fixed=2, n_points=60)
    e = imu[1:2]
    nsi, nsj = kfs["nav"][e[0]["kf_i"]].copy(), kfs["nav"][e[0]["kf_j"]].copy()
    nsi["dbg"], nsi["dba"] = [1e-3, -2e-3, 5e-4], [0.01, 0.02, -0.015]
    err0, J = oracle.lba_imu_edge_eval(params, e, nsi, nsj)
    h = 1e-6
    cols = [("i", 0, 6), ("j", 0, 6), ("i", 6, 3), ("j", 6, 3), ("i", 9, 6)]  # PR_i PR_j V_i V_j B_i
    c = 0
    for who, off, n in cols:
        for k in range(n):
            d = np.zeros(15)
            d[off + k] = h
            if who == "i":
                ep, _ = oracle.lba_imu_edge_eval(params, e, oracle.lba_navstate_inc(nsi, d), nsj, jac=False)
                em, _ = oracle.lba_imu_edge_eval(params, e, oracle.lba_navstate_inc(nsi, -d), nsj, jac=False)
            else:
                ep, _ = oracle.lba_imu_edge_eval(params, e, nsi, oracle.lba_navstate_inc(nsj, d), jac=False)
                em, _ = oracle.lba_imu_edge_eval(params, e, nsi, oracle.lba_navstate_inc(nsj, -d), jac=False)
            num = (ep[:9] - em[:9]) / (2 * h)
            assert np.allclose(num, J[:, c], atol=2e-5, rtol=1e-4), (c, num, J[:, c])
            c += 1
    assert c == 24
    # bias edge residual = (bg + dbg)_j - (bg + dbg)_i, (ba + dba)_j - (ba + dba)_i
    assert np.allclose(err0[9:12], (nsj["bg"] + nsj["dbg"]) - (nsi["bg"] + nsi["dbg"]))
    assert np.allclose(err0[12:15], (nsj["ba"] + nsj["dba"]) - (nsi["ba"] + nsi["dba"]))


def test_oracle_vio_lba_noiseless_recovers_truth(oracle):
    params, kfs, pts, close, obs, imu, gt = synth_ba.make_lba_vio_problem(
        5, n_points=500, outlier_frac=0.0, noise=0.0, stereo_frac=1.0, imu_noise=0.0)
    navs, pout, erase, res = oracle.local_ba_vio(params, kfs, pts, close, obs, imu)
    dp, dr, dv = _errs(navs, gt)
    assert res["status"] == 0 and res["n_erase"] == 0
    assert dp.max() < 5e-4 and dr.max() < 1e-4 and dv.max() < 2e-3
    assert res["chi2_final"] < 1e-3 * res["chi2_initial"]


def test_oracle_vio_lba_improves_state_and_rejects_outliers(oracle):
    params, kfs, pts, close, obs, imu, gt = synth_ba.make_lba_vio_problem(7, n_points=800)
    dp0, dr0, dv0 = _errs(kfs["nav"], gt)
    navs, pout, erase, res = oracle.local_ba_vio(params, kfs, pts, close, obs, imu)
    dp, dr, dv = _errs(navs, gt)
    assert res["status"] == 0
    assert dp.mean() < 0.5 * dp0.mean() and dv.mean() < 0.3 * dv0.mean()
    assert 0.01 < erase.mean() < 0.12  # 3 % planted gross outliers + the 5 % chi2 tail
    # biases are constants here: dbg/dba stay small, fixed key frames untouched
    n = gt["n_local"]
    assert np.abs(navs["dbg"][:n]).max() < 2e-3 and np.abs(navs["dba"][:n]).max() < 0.05
    assert navs[n:].tobytes() == kfs["nav"][n:].tobytes()


def test_oracle_vio_lba_edge_cases(oracle):
    params, kfs, pts, close, obs, imu, gt = synth_ba.make_lba_vio_problem(9, n_local=4, n_fixed=3, n_points=200)
    frozen = kfs.copy()
    frozen["fixed"] = 1
    navs, pout, erase, res = oracle.local_ba_vio(params, frozen, pts, close, obs, imu)
    assert res["status"] == 2 and np.array_equal(pout, pts) and not erase.any()
    navs, pout, erase, res = oracle.local_ba_vio(params, kfs, pts, close, obs, imu, stop=np.array([1], np.int32))
    assert res["status"] == 1 and res["lm_iterations"] == 0
    # divergence guard: a wrecked IMU measurement with the robust kernels off makes err_end > 2 err
    # unlikely to trigger on sane input; check instead that bLarge switches the guard off without changing the result
    p2 = params.copy()
    p2[0]["large"] = 1
    a = oracle.local_ba_vio(params, kfs, pts, close, obs, imu)
    b = oracle.local_ba_vio(p2, kfs, pts, close, obs, imu)
    assert a[3]["status"] == b[3]["status"] == 0 and a[0].tobytes() == b[0].tobytes()
    # first local key frame fixed (nid_ == 0), no key frame before the window
    params, kfs, pts, close, obs, imu, gt = synth_ba.make_lba_vio_problem(
        11, n_local=4, n_fixed=2, n_points=300, first_fixed=True, with_prev=False)
    navs, pout, erase, res = oracle.local_ba_vio(params, kfs, pts, close, obs, imu)
    assert np.array_equal(navs[0]["p"], kfs[0]["nav"]["p"]) and res["lm_iterations"] > 0


def _parity(oracle, win, hres):
    params, kfs, pts, close, obs, imu = win
    on, op, oe, ores = oracle.local_ba_vio(params, kfs, pts, close, obs, imu)
    hn, hp, he, hr = hres
    assert hr["status"] == ores["status"]
    if ores["status"] != 0:
        assert np.array_equal(hp, pts) and not he.any()
        return
    for k in range(len(kfs)):
        dt, dr = synth_ba.pose_error(on[k], hn[k])
        assert dt < 1e-4 and dr < 1e-4, (k, dt, dr)
        assert np.linalg.norm(on[k]["v"] - hn[k]["v"]) < 1e-4
        assert np.linalg.norm(on[k]["dbg"] - hn[k]["dbg"]) < 1e-6
        assert np.linalg.norm(on[k]["dba"] - hn[k]["dba"]) < 1e-5
    assert np.abs(op - hp).max() < 5e-2 and np.median(np.abs(op - hp)) < 2e-5
    assert (oe != he).mean() < 0.002
    assert abs(hr["chi2_final"] - ores["chi2_final"]) < 1e-5 * ores["chi2_final"] + 1e-2
    assert abs(hr["chi2_initial"] - ores["chi2_initial"]) < 1e-5 * ores["chi2_initial"]
    assert hr["lm_trials"] == ores["lm_trials"]


@pytest.mark.gpu
@pytest.mark.parametrize("seed,kw", [(20, {}), (21, dict(n_points=800)),
                                     (22, dict(n_local=5, n_fixed=3, n_points=400, stereo_frac=0.0)),
                                     (23, dict(n_local=4, n_fixed=2, n_points=300, first_fixed=True, with_prev=False)),
                                     (24, dict(n_local=13, n_fixed=6, n_points=1200))])
def test_gpu_vio_lba_parity(oracle, seed, kw):
    from vieo_slam_amd.optimizer import Optimizer
    win = synth_ba.make_lba_vio_problem(seed, **kw)[:6]
    _parity(oracle, win, Optimizer.LocalBundleAdjustmentNavStatePRV(*win))


@pytest.mark.gpu
def test_gpu_vio_lba_large_window_parity(oracle):
    """bLarge (Optimizer.cc:41-49, 131-138): Nlocal x 2.5 = 25 local key frames (375 unknowns: the reduced system no
    longer fits the LDS-resident solver's 132-dim panel form), optimize(2) + optimize(2), lambda_init 1e-2, no
    divergence guard"""
    from vieo_slam_amd.optimizer import Optimizer
    win = list(synth_ba.make_lba_vio_problem(26, n_local=25, n_fixed=8, n_points=2000, dt_kf=0.25)[:6])
    P = win[0].copy()
    P[0]["large"], P[0]["lambda_init"] = 1, 1e-2
    P[0]["base"]["its0"], P[0]["base"]["its1"] = 2, 2
    win[0] = P
    assert (win[1]["fixed"] == 0).sum() == 25
    _parity(oracle, tuple(win), Optimizer.LocalBundleAdjustmentNavStatePRV(*win))


@pytest.mark.gpu
@pytest.mark.parametrize("n_local", [10, 11, 21, 32, 42, 43])
def test_gpu_vio_lba_solver_classes_parity(oracle, n_local):
    """The one-workgroup L2-resident blocked LDL^T (k_lba_ldltg, 160 .. 639 unknowns): its smallest system (11 key
    frames = 165 unknowns, 11 blocks), a visual system whose last key frame straddles two 64-row Schur tiles (21 key
    frames: rows 126..131), 32 key frames (480 unknowns: more row blocks than gather wavefronts x 3) and its largest
    (42 key frames = 630 unknowns, 40 blocks); and the neighbours across the class boundaries: 10 key frames = 150
    unknowns (k_lba_ldlt16, LDS-resident) and 43 = 645 (the tiled k_big_* LDL^T over many workgroups)."""
    from vieo_slam_amd.optimizer import Optimizer
    win = list(synth_ba.make_lba_vio_problem(80 + n_local, n_local=n_local, n_fixed=6, n_points=1500, dt_kf=0.25)[:6])
    P = win[0].copy()
    P[0]["large"], P[0]["lambda_init"] = 1, 1e-2
    P[0]["base"]["its0"], P[0]["base"]["its1"] = 2, 2
    win[0] = P
    assert (win[1]["fixed"] == 0).sum() == n_local
    _parity(oracle, tuple(win), Optimizer.LocalBundleAdjustmentNavStatePRV(*win))


@pytest.mark.gpu
def test_gpu_vio_lba_mixed_batch_equals_single_calls():
    """Ordinary and bLarge windows in one lock-step batch (different Schur tile counts, K splits and solve kernels per
    window): every window's result is bit-identical to its own single-window call -- the summation orders are
    functions of the window alone."""
    from vieo_slam_amd.optimizer import Optimizer
    wins = []
    for i, n_local in enumerate([10, 25, 10, 12, 25]):
        w = list(synth_ba.make_lba_vio_problem(90 + i, n_local=n_local, n_fixed=8, n_points=900 + 150 * i, dt_kf=0.25)[:6])
        if n_local == 25:
            P = w[0].copy()
            P[0]["large"], P[0]["lambda_init"] = 1, 1e-2
            P[0]["base"]["its0"], P[0]["base"]["its1"] = 2, 2
            w[0] = P
        wins.append(tuple(w))
    outs = Optimizer.LocalBundleAdjustmentNavStatePRVBatch(wins)
    for win, (hn, hp, he, hr) in zip(wins, outs):
        sn, sp, se, sr = Optimizer.LocalBundleAdjustmentNavStatePRV(*win)
        assert hr["lm_trials"] == sr["lm_trials"] and hr["status"] == sr["status"]
        assert np.array_equal(hp, sp) and np.array_equal(he, se)
        for k in range(len(hn)):
            assert np.array_equal(hn[k]["p"], sn[k]["p"]) and np.array_equal(hn[k]["q"], sn[k]["q"])
            assert np.array_equal(hn[k]["v"], sn[k]["v"])


@pytest.mark.gpu
def test_gpu_vio_lba_batch_and_edge_cases(oracle):
    from vieo_slam_amd.optimizer import Optimizer
    wins = [synth_ba.make_lba_vio_problem(30 + i, n_local=4 + 3 * i, n_fixed=3, n_points=300 + 200 * i)[:6]
            for i in range(4)]
    frozen = wins[3][1].copy()
    frozen["fixed"] = 1
    wins[3] = (wins[3][0], frozen) + wins[3][2:]
    rec = wins[2][0].copy()
    rec[0]["rec_init"] = 1  # bRecInit: robust kernels on every inertial edge
    wins[2] = (rec,) + wins[2][1:]
    outs = Optimizer.LocalBundleAdjustmentNavStatePRVBatch(wins)
    for win, h in zip(wins, outs):
        _parity(oracle, win, h)
    hn, hp, he, hr = Optimizer.LocalBundleAdjustmentNavStatePRV(*wins[0], stop=np.array([1], np.int32))
    assert hr["status"] == 1 and hr["lm_iterations"] == 0 and np.array_equal(hp, wins[0][2])


@pytest.mark.gpu
def test_gpu_vio_lba_landmark_sharded_two_ranks_on_one_gpu(oracle):
    """Two 'ranks' (threads, each with its own stream and reduction buffer) run the landmark-sharded LBA
    of one window; the reduction callback sums the two buffers through the host.  The result must be the
    unsharded one (key frames identical on both ranks, each rank's points / erase flags = its shard)."""
    import threading
    from vieo_slam_amd import sharding
    from vieo_slam_amd._lib import DeviceBuffer, check, lib
    from vieo_slam_amd.optimizer import Optimizer
    win = synth_ba.make_lba_vio_problem(50, n_local=6, n_fixed=3, n_points=600)[:6]
    on, op, oe, ores = oracle.local_ba_vio(*win)
    world = 2
    shards = [sharding.shard_window(win, r, world) for r in range(world)]
    n = Optimizer.sharded_buffer_doubles([shards[0][0]])
    bufs = [DeviceBuffer(8 * n) for _ in range(world)]
    barrier = threading.Barrier(world)
    stage = [None] * world
    results = [None] * world

    def make_cb(rank):
        def cb(offset, count):
            h = np.empty(count)
            check(lib().vieo_memcpy_d2h(h.ctypes.data, bufs[rank].ptr + 8 * offset, 8 * count))
            stage[rank] = h
            barrier.wait()
            total = stage[0] + stage[1]
            barrier.wait()
            check(lib().vieo_memcpy_h2d(bufs[rank].ptr + 8 * offset, total.ctypes.data, 8 * count))
            return 0
        return cb

    def run(rank):
        results[rank] = Optimizer.LocalBundleAdjustmentNavStatePRVSharded([shards[rank][0]], bufs[rank].ptr, n,
                                                                          make_cb(rank))[0]
    ts = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [t.start() for t in ts]
    [t.join(120) for t in ts]
    assert all(r is not None for r in results)
    for rank in range(world):
        hn, hp, he, hr = results[rank]
        mine = shards[rank][1]
        assert hr["status"] == 0 and hr["lm_trials"] == ores["lm_trials"]
        for k in range(len(win[1])):
            dt, dr = synth_ba.pose_error(on[k], hn[k])
            assert dt < 1e-4 and dr < 1e-4 and np.linalg.norm(on[k]["v"] - hn[k]["v"]) < 1e-4
        assert np.abs(op[mine] - hp).max() < 5e-2 and np.median(np.abs(op[mine] - hp)) < 2e-5
        sel = np.isin(win[4]["mp"], mine)
        assert (oe[sel] != he).mean() < 0.004
        assert abs(hr["chi2_final"] - ores["chi2_final"]) < 1e-5 * ores["chi2_final"] + 1e-2
    assert results[0][0].tobytes() == results[1][0].tobytes()  # replicated solve: bit-identical key frames
    # world = 1: the sharded entry with a no-op reduction equals the plain call
    n1 = Optimizer.sharded_buffer_doubles([win])
    b1 = DeviceBuffer(8 * n1)
    s1 = Optimizer.LocalBundleAdjustmentNavStatePRVSharded([win], b1.ptr, n1, lambda off, cnt: 0)[0]
    p1 = Optimizer.LocalBundleAdjustmentNavStatePRV(*win)
    assert s1[0].tobytes() == p1[0].tobytes() and np.array_equal(s1[1], p1[1]) and np.array_equal(s1[2], p1[2])


def _run_ranks(world, shards, n, bad_rank=None, stops=None, on_exchange=None):
    """world 'ranks' as host threads on one GPU; the reduction callback sums their buffers through the host"""
    import threading
    from vieo_slam_amd._lib import DeviceBuffer, VieoError, check, lib
    from vieo_slam_amd.optimizer import Optimizer
    bufs = [DeviceBuffer(8 * n) for _ in range(world)]
    barrier = threading.Barrier(world)
    stage, results = [None] * world, [None] * world

    def make_cb(rank):
        def cb(offset, count):
            h = np.empty(count)
            check(lib().vieo_memcpy_d2h(h.ctypes.data, bufs[rank].ptr + 8 * offset, 8 * count))
            stage[rank] = h
            if on_exchange:
                on_exchange(rank, count)
            barrier.wait(60)
            total = sum(stage[r] for r in range(world))
            barrier.wait(60)
            check(lib().vieo_memcpy_h2d(bufs[rank].ptr + 8 * offset, total.ctypes.data, 8 * count))
            return 0
        return cb

    def run(rank):
        try:
            results[rank] = Optimizer.LocalBundleAdjustmentNavStatePRVSharded([shards[rank]], bufs[rank].ptr, n,
                                                                              make_cb(rank),
                                                                              stop=None if stops is None else stops[rank])[0]
        except VieoError as e:
            results[rank] = e
    ts = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [t.start() for t in ts]
    [t.join(120) for t in ts]
    assert not any(t.is_alive() for t in ts), "a rank hangs in the exchange"
    return results


@pytest.mark.gpu
def test_gpu_vio_lba_sharded_empty_shard_and_collective_abort(oracle):
    """A rank may own no point of a window (more ranks than points, or points without observations): it contributes
    zeros and still takes part in every exchange.  And when one rank's arguments are invalid, ALL ranks return
    VIEO_E_INVALID together instead of leaving the others waiting in the all-reduce."""
    from vieo_slam_amd import sharding
    from vieo_slam_amd._lib import VieoError
    from vieo_slam_amd.optimizer import Optimizer
    win = synth_ba.make_lba_vio_problem(52, n_local=5, n_fixed=2, n_points=300)[:6]
    ref = Optimizer.LocalBundleAdjustmentNavStatePRV(*win)
    two = [sharding.shard_window(win, r, 2) for r in range(2)]
    params, kfs, points, close, obs, imu = win
    empty = (params, kfs, points[:0].copy(), np.asarray(close)[:0].copy(), obs[:0].copy(), imu)
    shards = [two[0][0], two[1][0], empty]
    n = Optimizer.sharded_buffer_doubles([two[0][0]])
    res = _run_ranks(3, shards, n)
    assert all(not isinstance(r, Exception) for r in res), res
    for rank in range(3):
        hn, hp, he, hr = res[rank]
        assert hr["status"] == 0 and hr["lm_trials"] == ref[3]["lm_trials"]
        for k in range(len(kfs)):
            dt, dr = synth_ba.pose_error(ref[0][k], hn[k])
            assert dt < 1e-6 and dr < 1e-6
    assert res[0][0].tobytes() == res[1][0].tobytes() == res[2][0].tobytes()
    assert len(res[2][1]) == 0 and len(res[2][2]) == 0
    # rank 1 hands in unsorted observations: every rank comes back with an error, nobody hangs
    bad = list(two[1][0])
    bad[4] = bad[4][::-1].copy()
    res = _run_ranks(2, [two[0][0], tuple(bad)], n)
    assert all(isinstance(r, VieoError) for r in res), res
    assert "another rank" in str(res[0]) and "this rank" in str(res[1])
    # a failure only one rank runs into AFTER the argument agreement (a singular pre-integration covariance met while
    # staging): it reports to the second agreement on its way out, the other rank returns too
    bad = list(two[1][0])
    bad[5] = bad[5].copy()
    bad[5]["imu"]["Sigma"][0] = 0.0
    res = _run_ranks(2, [two[0][0], tuple(bad)], n)
    assert all(isinstance(r, VieoError) for r in res), res
    assert "staging" in str(res[0]) and "singular" in str(res[1])
    # ... and the engine is fine afterwards
    res = _run_ranks(2, [two[0][0], two[1][0]], n)
    assert all(not isinstance(r, Exception) for r in res) and res[0][3]["lm_trials"] == ref[3]["lm_trials"]


@pytest.mark.gpu
def test_gpu_vio_lba_in_library_rccl_single_rank():
    """The dlopen'ed RCCL path (vieo_rccl_*): a one-rank communicator, ncclAllReduce issued by the library on its own
    stream between the pack and assemble kernels; with one rank the result is the plain call's, bit for bit."""
    from vieo_slam_amd import sharding
    from vieo_slam_amd._lib import DeviceBuffer, lib
    from vieo_slam_amd.optimizer import Optimizer
    assert lib().vieo_rccl_available() == 1
    win = synth_ba.make_lba_vio_problem(53, n_local=6, n_fixed=3, n_points=500)[:6]
    comm = sharding.RcclComm(0, 1)
    try:
        n = Optimizer.sharded_buffer_doubles([win])
        buf = DeviceBuffer(8 * n)
        s = Optimizer.LocalBundleAdjustmentNavStatePRVSharded([win], buf.ptr, n, comm=comm.handle)[0]
        p = Optimizer.LocalBundleAdjustmentNavStatePRV(*win)
        assert s[3]["status"] == 0 and s[0].tobytes() == p[0].tobytes()
        assert np.array_equal(s[1], p[1]) and np.array_equal(s[2], p[2])
    finally:
        comm.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rig,seed", [("radtan", 70), ("kb8", 71)])
def test_gpu_vio_lba_distorted_rig_parity(oracle, rig, seed):
    """a18 on a distorted multi-camera rig (a20): per-observation camera, Radtan / KB8 projection."""
    from vieo_slam_amd.optimizer import Optimizer
    w = synth_ba.make_lba_vio_problem(seed, n_local=6, n_fixed=3, n_points=500, rig=rig)
    win = w[:6]
    _parity(oracle, win, Optimizer.LocalBundleAdjustmentNavStatePRV(*win))


def test_oracle_th_dist_far_excludes_far_monocular_points(oracle):
    """th_dist_far (Optimizer.cc:395,454,513-517): points no monocular edge sees closer than the limit lose their
    monocular edges; chi2 of the first linearisation drops with the excluded edges, stereo-only windows are untouched."""
    import numpy as np
    win = synth_ba.make_lba_vio_problem(31, n_points=600, stereo_frac=0.3)[:6]
    base = oracle.local_ba_vio(*win)[3]
    far = [w.copy() if hasattr(w, "copy") else w for w in win]
    far[0][0]["th_dist_far"] = 5.0
    r5 = oracle.local_ba_vio(*far)[3]
    far[0][0]["th_dist_far"] = 1e-3  # nothing is that close: every monocular edge goes
    r0 = oracle.local_ba_vio(*far)[3]
    far[0][0]["th_dist_far"] = np.inf
    rinf = oracle.local_ba_vio(*far)[3]
    assert r0["chi2_initial"] < r5["chi2_initial"] < base["chi2_initial"]
    assert rinf["chi2_initial"] == base["chi2_initial"]
    st = list(synth_ba.make_lba_vio_problem(32, n_points=400, stereo_frac=1.0)[:6])
    st[4] = st[4].copy()
    st[4]["ur"] = np.abs(st[4]["ur"])  # (a stereo coordinate left of the image would make the edge monocular)
    a = oracle.local_ba_vio(*st)[3]
    st[0][0]["th_dist_far"] = 3.0
    assert oracle.local_ba_vio(*st)[3]["chi2_initial"] == a["chi2_initial"]


@pytest.mark.gpu
@pytest.mark.parametrize("th", [3.0, 6.0, 1e-3])
def test_gpu_vio_lba_th_dist_far_parity(oracle, th):
    from vieo_slam_amd.optimizer import Optimizer
    win = list(synth_ba.make_lba_vio_problem(33, n_points=700, stereo_frac=0.4)[:6])
    win[0][0]["th_dist_far"] = th
    _parity(oracle, win, Optimizer.LocalBundleAdjustmentNavStatePRV(*win))


# ------------------------------------------------------------------ encoder edges (EdgeEncNavStatePR)
def test_oracle_encoder_edge_residual_and_jacobians(oracle):
    """g2otypes.h:606-665: zero residual for a consistent measurement; Jacobians against central differences of
    computeError through the PR vertex's oplus (p += R dp, R *= Exp(dphi))."""
    import numpy as np
    params, kfs, pts, close, obs, imu, gt = synth_ba.make_lba_vio_problem(3, n_local=3, n_fixed=2, n_points=60,
                                                                          enc=True)
    e = imu[1]
    qbe, pbe = params[0]["qRbe"], params[0]["pbe"]
    nsi, nsj = kfs["nav"][e["kf_i"]].copy(), kfs["nav"][e["kf_j"]].copy()
    # at the true states the residual is the measurement noise
    ti, tj = nsi.copy(), nsj.copy()
    ti["p"], ti["q"], tj["p"], tj["q"] = gt["p"][e["kf_i"]], gt["q"][e["kf_i"]], gt["p"][e["kf_j"]], gt["q"][e["kf_j"]]
    err, _, _ = oracle.enc_edge_eval(ti, tj, e["enc"]["delx"], qbe, pbe, jac=False)
    assert np.abs(err[:3]).max() < 0.01 and np.abs(err[3:]).max() < 0.03
    err0, Ji, Jj = oracle.enc_edge_eval(nsi, nsj, e["enc"]["delx"], qbe, pbe)
    h = 1e-6
    for who, J in (("i", Ji), ("j", Jj)):
        for k in range(6):
            d = np.zeros(15)
            d[k] = h
            if who == "i":
                ep, _, _ = oracle.enc_edge_eval(oracle.lba_navstate_inc(nsi, d), nsj, e["enc"]["delx"], qbe, pbe, False)
                em, _, _ = oracle.enc_edge_eval(oracle.lba_navstate_inc(nsi, -d), nsj, e["enc"]["delx"], qbe, pbe, False)
            else:
                ep, _, _ = oracle.enc_edge_eval(nsi, oracle.lba_navstate_inc(nsj, d), e["enc"]["delx"], qbe, pbe, False)
                em, _, _ = oracle.enc_edge_eval(nsi, oracle.lba_navstate_inc(nsj, -d), e["enc"]["delx"], qbe, pbe, False)
            assert np.allclose((ep - em) / (2 * h), J[:, k], atol=2e-6, rtol=1e-5), (who, k)


def test_oracle_vio_lba_with_encoder_edges(oracle):
    win = synth_ba.make_lba_vio_problem(41, n_points=500, enc=True)
    navs, pout, erase, res = oracle.local_ba_vio(*win[:6])
    dp, dr, dv = _errs(navs, win[6])
    dp0, dr0, dv0 = _errs(win[1]["nav"], win[6])
    assert res["status"] == 0 and dr.mean() < 0.5 * dr0.mean() and res["chi2_final"] < 0.1 * res["chi2_initial"]
    # the edges take part: dropping them changes the cost
    no = list(win[:6])
    no[5] = no[5].copy()
    no[5]["enc"]["dt"] = 0
    assert oracle.local_ba_vio(*no)[3]["chi2_initial"] < res["chi2_initial"]


@pytest.mark.gpu
@pytest.mark.parametrize("seed,kw", [(42, {}), (43, dict(n_local=5, n_fixed=3, n_points=400, with_prev=False,
                                                         first_fixed=True))])
def test_gpu_vio_lba_encoder_parity(oracle, seed, kw):
    from vieo_slam_amd.optimizer import Optimizer
    win = synth_ba.make_lba_vio_problem(seed, enc=True, **kw)[:6]
    _parity(oracle, win, Optimizer.LocalBundleAdjustmentNavStatePRV(*win))


@pytest.mark.gpu
@pytest.mark.parametrize("robust", [True, False])
def test_gpu_vio_gba_encoder_parity(oracle, robust):
    import numpy as np
    from vieo_slam_amd.optimizer import Optimizer
    params, kfs, pts, close, obs, imu, gt = synth_ba.make_lba_vio_problem(44, n_local=40, n_fixed=1, n_points=3000,
                                                                          anchors=20, span=5, enc=True)
    on, op, ores = oracle.global_ba_vio(params, kfs, pts, obs, imu, 5, robust)
    hn, hp, hres = Optimizer.GlobalBundleAdjustmentNavStatePRV(params, kfs, pts, obs, imu, 5, robust)
    for k in range(40):
        dt, dr = synth_ba.pose_error(on[k], hn[k])
        assert dt < 1e-4 and dr < 1e-4, (k, dt, dr)
    assert hres["lm_trials"] == ores["lm_trials"]
    assert abs(hres["chi2_final"] - ores["chi2_final"]) <= 1e-6 * ores["chi2_final"]


@pytest.mark.gpu
@pytest.mark.parametrize("i", [0, 3, 7])
def test_gpu_vio_lba_bench_windows_parity(oracle, i):
    """The local-BA windows of bench.py's timed step EXACTLY as it builds them (workload r3, SURVEY 8d: 10 local + 40
    fixed key frames, ~1500 points / ~21 k observations; every 4th window bLarge -- 25 local key frames, optimize(2) +
    optimize(2)) against the oracle: the shapes the headline is measured on."""
    from vieo_slam_amd.optimizer import Optimizer
    large = i % 4 == 3
    w = synth_ba.make_lba_vio_problem(500 + i, n_local=25 if large else 10, n_fixed=40, n_points=2000)[:6]
    w[0][0]["large"] = int(large)
    if large:
        w[0][0]["base"]["its0"], w[0][0]["base"]["its1"] = 2, 2
    assert (w[1]["fixed"] != 0).sum() >= 40 and len(w[4]) > 15000
    _parity(oracle, w, Optimizer.LocalBundleAdjustmentNavStatePRV(*w))


@pytest.mark.gpu
def test_gpu_vio_lba_sharded_stop_flag_is_collective(oracle):
    """pbStopFlag of a landmark-sharded local BA (Optimizer.cc:524-528,570-571): the flag is rank-local, the ranks' requests
    are summed inside the run's own exchanges -- raised on ONE rank, before the call or in the middle of it, it stops ALL
    ranks at the same trial (nobody hangs in a collective), with the status and the key frames the same on every rank."""
    from vieo_slam_amd import sharding
    from vieo_slam_amd.optimizer import Optimizer
    win = synth_ba.make_lba_vio_problem(58, n_local=6, n_fixed=3, n_points=600)[:6]
    world = 3
    shards = [sharding.shard_window(win, r, world)[0] for r in range(world)]
    n = Optimizer.sharded_buffer_doubles([shards[0]])
    full = _run_ranks(world, shards, n)
    assert all(r[3]["status"] == 0 for r in full)
    # raised on rank 1 before the call: every rank returns the aborted status with nothing optimised
    stops = [np.zeros(1, np.int32) for _ in range(world)]
    stops[1][0] = 1
    res = _run_ranks(world, shards, n, stops=stops)
    plain_stop = np.ones(1, np.int32)
    ref = Optimizer.LocalBundleAdjustmentNavStatePRV(*win, stop=plain_stop)
    for r in res:
        assert not isinstance(r, Exception) and int(r[3]["status"]) == int(ref[3]["status"]) != 0
        assert r[0].tobytes() == ref[0].tobytes() and int(r[3]["lm_trials"]) == 0
    # raised on rank 2 in the middle (after its 4th trial exchange): all ranks stop together, earlier than the full run
    stops = [np.zeros(1, np.int32) for _ in range(world)]
    seen = [0]

    def on_exchange(rank, count):
        if rank == 2 and count == 4:  # (the 4-scalar exchange of a trial)
            seen[0] += 1
            if seen[0] == 4:
                stops[2][0] = 1
    res = _run_ranks(world, shards, n, stops=stops, on_exchange=on_exchange)
    trials = [int(r[3]["lm_trials"]) for r in res]
    assert len(set(trials)) == 1 and 4 <= trials[0] < int(full[0][3]["lm_trials"]), (trials, int(full[0][3]["lm_trials"]))
    assert res[0][0].tobytes() == res[1][0].tobytes() == res[2][0].tobytes()


@pytest.mark.gpu
def test_gpu_lba_stream_priority_changes_nothing_but_the_stream():
    """vieo_lba_set_stream_priority: -1 / 0 / 1 are accepted (anything else is VIEO_E_INVALID), the calling thread's stream is
    made again at the next call, and the solve returns the same bytes whatever its stream's priority."""
    from vieo_slam_amd._lib import lib
    from vieo_slam_amd.optimizer import Optimizer
    L = lib()
    win = synth_ba.make_lba_vio_problem(31, n_local=6, n_fixed=3, n_points=500)[:6]
    assert L.vieo_lba_set_stream_priority(2) != 0 and L.vieo_lba_set_stream_priority(-2) != 0
    outs = []
    for pr in (-1, 0, 1, -1):
        assert L.vieo_lba_set_stream_priority(pr) == 0
        n, p, e, r = Optimizer.LocalBundleAdjustmentNavStatePRV(*win)
        outs.append((n.tobytes(), p.tobytes(), e.tobytes(), int(r["lm_trials"])))
    assert all(o == outs[0] for o in outs[1:])
