"""Pose-graph optimisation on the device (reference Optimizer::OptimizeEssentialGraph, src/Optimizer.cc:2309-2687, the
numeric call of LoopClosing::CorrectLoop): the numpy dtypes of the records of include/vieo_hot.h,
optimize_essential_graph -- vieo_optimize_essential_graph --, linearize and solve -- the test taps
vieo_pose_graph_linearize and vieo_pose_graph_solve --,
essential_graph_edges -- the reference's edge selection (:2395-2617) from flat arrays --, and make_loop_trajectory, the
generator of the tests and of tools/time_pose_graph.py."""
import math

import numpy as np

from . import _lib

SIM3_DTYPE = np.dtype([("q", np.float64, 4), ("t", np.float64, 3), ("s", np.float64)], align=True)
POSE_GRAPH_DTYPE = np.dtype([("n_kf", np.int32), ("n_edges", np.int32), ("n_mp", np.int32), ("fixed_kf", np.int32),
                             ("fix_scale", np.int32), ("n_iterations", np.int32), ("lambda_init", np.float64),
                             ("valid", np.uint64), ("Scw", np.uint64), ("Scw_prior", np.uint64), ("edge_i", np.uint64),
                             ("edge_j", np.uint64), ("edge_kind", np.uint64), ("edge_info", np.uint64), ("Pw", np.uint64),
                             ("ref_kf", np.uint64)], align=True)
PG_TRIAL_DTYPE = np.dtype([("chi2_before", np.float64), ("chi2_after", np.float64), ("lambda", np.float64),
                           ("accepted", np.int32), ("solved", np.int32)], align=True)
POSE_GRAPH_RESULT_DTYPE = np.dtype([("status", np.int32), ("n_unknowns", np.int32), ("lm_iterations", np.int32),
                                    ("lm_trials", np.int32), ("chi2_initial", np.float64), ("chi2_final", np.float64),
                                    ("n_trace", np.int32), ("trace_cap", np.int32), ("Scw_opt", np.uint64),
                                    ("Tcw", np.uint64), ("Pw_out", np.uint64), ("Pw_out_d", np.uint64), ("trace", np.uint64),
                                    ("bytes_needed", np.uint64)], align=True)

EDGE_LOOP, EDGE_PRIOR = 0, 1
MIN_FEAT = 100  # Optimizer.cc:2347


def sim3_array(q, t, s=None):
    """(n, 4) quaternions x, y, z, w + (n, 3) translations (+ scales) -> SIM3_DTYPE[n]"""
    q = np.asarray(q, np.float64).reshape(-1, 4)
    out = np.zeros(len(q), SIM3_DTYPE)
    out["q"], out["t"] = q, np.asarray(t, np.float64).reshape(-1, 3)
    out["s"] = 1.0 if s is None else s
    return out


class _Graph:
    """the vieo_pose_graph record with the arrays it points to kept alive"""

    def __init__(self, Scw, Scw_prior, valid, fixed_kf, edge_i, edge_j, edge_kind, edge_info, Pw, ref_kf, fix_scale,
                 n_iterations, lambda_init):
        self.Scw = np.ascontiguousarray(Scw, SIM3_DTYPE)
        self.Scw_prior = self.Scw if Scw_prior is None else np.ascontiguousarray(Scw_prior, SIM3_DTYPE)
        n = len(self.Scw)
        self.valid = np.ones(n, np.uint8) if valid is None else np.ascontiguousarray(valid, np.uint8)
        self.edge_i = np.ascontiguousarray(edge_i, np.int32).reshape(-1)
        self.edge_j = np.ascontiguousarray(edge_j, np.int32).reshape(-1)
        ne = len(self.edge_i)
        self.edge_kind = np.ascontiguousarray(edge_kind, np.int32).reshape(-1)
        self.edge_info = (np.ones((ne, 2)) if edge_info is None else np.ascontiguousarray(edge_info, np.float64)).reshape(-1, 2)
        self.Pw = np.zeros((0, 3), np.float32) if Pw is None else np.ascontiguousarray(Pw, np.float32).reshape(-1, 3)
        self.ref_kf = np.zeros(0, np.int32) if ref_kf is None else np.ascontiguousarray(ref_kf, np.int32).reshape(-1)
        if not (len(self.Scw_prior) == len(self.valid) == n and len(self.edge_j) == len(self.edge_kind) == ne and
                len(self.edge_info) == ne and len(self.ref_kf) == len(self.Pw)):
            raise ValueError("pose graph: array lengths differ")
        r = np.zeros(1, POSE_GRAPH_DTYPE)
        r["n_kf"], r["n_edges"], r["n_mp"], r["fixed_kf"] = n, ne, len(self.Pw), fixed_kf
        r["fix_scale"], r["n_iterations"], r["lambda_init"] = int(bool(fix_scale)), n_iterations, lambda_init
        for name in ("valid", "Scw", "Scw_prior", "edge_i", "edge_j", "edge_kind", "edge_info", "Pw", "ref_kf"):
            arr = getattr(self, name)
            if arr.size:
                r[name] = arr.ctypes.data
        self.rec = r


def optimize_essential_graph_call(Scw, Scw_prior, valid, fixed_kf, edge_i, edge_j, edge_kind, edge_info=None, Pw=None,
                                  ref_kf=None, fix_scale=True, n_iterations=20, lambda_init=1e-16, trace_cap=256,
                                  tap_points=False):
    """vieo_optimize_essential_graph, raw: (rc, dict).  The outputs are pre-filled with a pattern so that a caller can see
    what a refused call left untouched."""
    g = _Graph(Scw, Scw_prior, valid, fixed_kf, edge_i, edge_j, edge_kind, edge_info, Pw, ref_kf, fix_scale, n_iterations,
               lambda_init)
    n, nmp = len(g.Scw), len(g.Pw)
    Scw_opt = np.zeros(n, SIM3_DTYPE)
    Scw_opt["s"] = -7.0
    Tcw = np.full((n, 3, 4), -7.0)
    Pw_out = np.full((max(nmp, 1), 3), -7.0, np.float32)
    Pw_out_d = np.full((max(nmp, 1), 3), -7.0) if tap_points else None
    trace = np.zeros(max(trace_cap, 1), PG_TRIAL_DTYPE)
    res = np.zeros(1, POSE_GRAPH_RESULT_DTYPE)
    res["status"], res["trace_cap"] = -99, trace_cap
    res["Scw_opt"], res["Tcw"], res["Pw_out"], res["trace"] = Scw_opt.ctypes.data, Tcw.ctypes.data, Pw_out.ctypes.data, trace.ctypes.data
    if tap_points:
        res["Pw_out_d"] = Pw_out_d.ctypes.data
    rc = _lib.lib().vieo_optimize_essential_graph(g.rec.ctypes.data, res.ctypes.data)
    r = res[0]
    return rc, dict(status=int(r["status"]), n_unknowns=int(r["n_unknowns"]), lm_iterations=int(r["lm_iterations"]),
                    lm_trials=int(r["lm_trials"]), chi2_initial=float(r["chi2_initial"]), chi2_final=float(r["chi2_final"]),
                    bytes_needed=int(r["bytes_needed"]), Scw_opt=Scw_opt, Tcw=Tcw, Pw_out=Pw_out[:nmp],
                    Pw_out_d=None if Pw_out_d is None else Pw_out_d[:nmp], trace=trace[:int(r["n_trace"])].copy())


def optimize_essential_graph(Scw, Scw_prior, valid, fixed_kf, edge_i, edge_j, edge_kind, edge_info=None, Pw=None, ref_kf=None,
                             fix_scale=True, n_iterations=20, lambda_init=1e-16, trace_cap=256):
    """void Optimizer::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections,
    bFixScale), flattened: Scw = vScw (SIM3_DTYPE per key frame in nid_ order: the corrected Sim3 where there is one, else
    (Rcw, tcw, 1)), Scw_prior = the NonCorrectedSim3 entry where there is one (None: Scw), valid = !isBad(), fixed_kf =
    pLoopKF, the edges of essential_graph_edges, Pw / ref_kf the map points with their nIDr (-1: bad).
    returns dict(Scw_opt, Tcw (n, 3, 4) = R | t / s, Pw_out, lm_iterations, lm_trials, chi2_initial, chi2_final, trace)."""
    rc, out = optimize_essential_graph_call(Scw, Scw_prior, valid, fixed_kf, edge_i, edge_j, edge_kind, edge_info, Pw, ref_kf,
                                            fix_scale, n_iterations, lambda_init, trace_cap)
    _lib.check(rc, "vieo_optimize_essential_graph")
    return out


def linearize(Scw, Scw_prior, valid, fixed_kf, edge_i, edge_j, edge_kind, edge_info=None, fix_scale=True):
    """test tap: (e (n, 7), Ji (n, 7, 7), Jj (n, 7, 7)) of every edge at the estimates Scw"""
    g = _Graph(Scw, Scw_prior, valid, fixed_kf, edge_i, edge_j, edge_kind, edge_info, None, None, fix_scale, 0, 0.0)
    ne = len(g.edge_i)
    e, Ji, Jj = np.zeros((max(ne, 1), 7)), np.zeros((max(ne, 1), 7, 7)), np.zeros((max(ne, 1), 7, 7))
    _lib.check(_lib.lib().vieo_pose_graph_linearize(g.rec.ctypes.data, e.ctypes.data, Ji.ctypes.data, Jj.ctypes.data),
               "vieo_pose_graph_linearize")
    return e[:ne], Ji[:ne], Jj[:ne]


def free_key_frames(valid, fixed_kf, edge_i, edge_j):
    """the key frames that are unknowns, in the order of their columns: valid, not the fixed one, with an edge"""
    valid = np.asarray(valid).astype(bool)
    deg = np.bincount(np.concatenate([np.asarray(edge_i, np.int64), np.asarray(edge_j, np.int64)]), minlength=len(valid))
    return np.flatnonzero(valid & (deg[:len(valid)] > 0) & (np.arange(len(valid)) != fixed_kf))


def solve(Scw, Scw_prior, valid, fixed_kf, edge_i, edge_j, edge_kind, edge_info=None, fix_scale=True, lam=0.0):
    """test tap: one assemble + factorisation + back substitution at the estimates Scw.
    returns dict(x (n,), b (n,), H_lower (n, n), ok, free_kf) with n = (6 or 7) x len(free_kf)"""
    g = _Graph(Scw, Scw_prior, valid, fixed_kf, edge_i, edge_j, edge_kind, edge_info, None, None, fix_scale, 0, 0.0)
    free = free_key_frames(g.valid, fixed_kf, g.edge_i, g.edge_j)
    n = len(free) * (6 if fix_scale else 7)
    x, b, H = np.full(max(n, 1), -7.0), np.full(max(n, 1), -7.0), np.full((max(n, 1), max(n, 1)), -7.0)
    ok = np.full(1, -7, np.int32)
    _lib.check(_lib.lib().vieo_pose_graph_solve(g.rec.ctypes.data, float(lam), x.ctypes.data, b.ctypes.data, H.ctypes.data,
                                                ok.ctypes.data), "vieo_pose_graph_solve")
    return dict(x=x[:n], b=b[:n], H_lower=H[:n, :n] if n else np.zeros((0, 0)), ok=int(ok[0]), free_kf=free)


# ---------------------------------------------------------------------------------------------------------------------
def essential_graph_edges(valid, parent, loop_edges, covisibility, loop_connections, cur_kf, loop_kf, children=None,
                          odom_sigma_base=None, odom_sigma_edge=None, min_feat=MIN_FEAT):
    """The edges Optimizer::OptimizeEssentialGraph adds (Optimizer.cc:2395-2617), from flat descriptions of the map:

      valid[n]          !isBad() per key frame, index = nid_
      parent[n]         GetParent(), -1 for none
      loop_edges        pairs (a, b): b is in a's GetLoopEdges() (listed in both directions if the map holds both)
      covisibility      rows (i, j, w): j is in i's mvpOrderedConnectedKeyFrames with weight w, the rows of one i in that
                        list's order (GetCovisiblesByWeight keeps its prefix with w >= min_feat; GetWeight(i, j) = w, 0 for
                        a pair without a row)
      loop_connections  {i: iterable of j}: LoopConnections; walked in ascending nid_ (the reference walks its std::map and
                        std::set by pointer value, which only permutes equal-rank summands)
      children          {p: set}: hasChild(); None: derived from parent
      odom_sigma_base   {kf: (sigma_phi, sigma_p)} for the key frames whose spanning-tree edge is a pure odometry edge
                        under the state / GetPrevKeyFrame condition of :2438-2439: the two dTmp of :2452-2461
      odom_sigma_edge   the same for the two fSigmaOdom of :2524-2534 (the reference picks the pre-integrator by another
                        rule there); None: odom_sigma_base

    returns (edge_i, edge_j, edge_kind, edge_info (n, 2)) in the reference's order of addEdge.  Kept from the reference:
    the (cur_kf, loop_kf) pair enters whatever its weight; sInsertedEdges keeps a covisibility edge out that is already a
    new loop connection, but neither a spanning-tree nor an old loop edge (a parent that is a loop connection is added
    twice); old loop and covisibility edges only towards the lower nid_; a covisibility edge to the parent, to a child or
    to an old loop edge's other end is left out; fOdomBase in float, elemInfo == 0 or > 1e6 -> 1; matLambdaOdom is one
    matrix declared ahead of the loop and rewritten block by block (both blocks are rewritten whenever it is used, so the
    value it carries over is never seen in an edge)."""
    valid = np.asarray(valid).astype(bool)
    n = len(valid)
    parent = np.asarray(parent, np.int64)
    weight, ordered = {}, {}
    for i, j, w in covisibility:
        weight[(int(i), int(j))] = int(w)
        ordered.setdefault(int(i), []).append((int(j), int(w)))
    loops = {}
    for a, b in loop_edges:
        loops.setdefault(int(a), set()).add(int(b))
    if children is None:
        children = {}
        for k in range(n):
            if parent[k] >= 0:
                children.setdefault(int(parent[k]), set()).add(k)
    odom_sigma_base = odom_sigma_base or {}
    odom_sigma_edge = odom_sigma_base if odom_sigma_edge is None else odom_sigma_edge
    ei, ej, kind, info = [], [], [], []

    def add(i, j, k, w=(1.0, 1.0)):
        if not (0 <= i < n and 0 <= j < n and valid[i] and valid[j]):
            raise ValueError("essential_graph_edges: edge (%d, %d) names a bad key frame" % (i, j))
        ei.append(i), ej.append(j), kind.append(k), info.append(w)

    inserted = set()
    for i in sorted(int(k) for k in loop_connections):
        for j in sorted(int(k) for k in loop_connections[i]):
            if (i != cur_kf or j != loop_kf) and weight.get((i, j), 0) < min_feat:
                continue
            add(i, j, EDGE_LOOP)
            inserted.add((min(i, j), max(i, j)))
    base = [np.float32(1), np.float32(1)]
    for k in range(n):
        if valid[k] and parent[k] >= 0 and weight.get((k, int(parent[k])), 0) < min_feat and k in odom_sigma_base:
            for c in range(2):
                if float(base[c]) > float(odom_sigma_base[k][c]):
                    base[c] = np.float32(odom_sigma_base[k][c])
    lam_odom = [1.0, 1.0]  # matLambdaOdom's two blocks
    for k in range(n):
        if not valid[k]:
            continue
        p = int(parent[k])
        if p >= 0:
            w = (1.0, 1.0)
            if weight.get((k, p), 0) < min_feat and k in odom_sigma_edge:
                for c in range(2):
                    with np.errstate(divide="ignore", invalid="ignore"):
                        elem = np.float32(base[c]) / np.float32(odom_sigma_edge[k][c])
                    lam_odom[c] = 1.0 if (elem == 0 or elem > np.float32(1e6)) else float(elem)
                w = (lam_odom[0], lam_odom[1])
            add(k, p, EDGE_PRIOR, w)
        mine = loops.get(k, set())
        for l in sorted(mine):
            if l < k:
                add(k, l, EDGE_PRIOR)
        for j, w in ordered.get(k, []):
            if w < min_feat:
                break
            if j != p and j not in children.get(k, set()) and j not in mine and valid[j] and j < k:
                if (min(k, j), max(k, j)) in inserted:
                    continue
                add(k, j, EDGE_PRIOR)
    return (np.array(ei, np.int32), np.array(ej, np.int32), np.array(kind, np.int32),
            np.array(info, np.float64).reshape(-1, 2))


# ---------------------------------------------------------------------------------------------------------------------
def _quat_from_rotvec(w):
    th = float(np.linalg.norm(w))
    if th < 1e-12:
        return np.array([0.5 * w[0], 0.5 * w[1], 0.5 * w[2], 1.0])
    a = np.asarray(w, np.float64) / th
    return np.array([a[0] * math.sin(th / 2), a[1] * math.sin(th / 2), a[2] * math.sin(th / 2), math.cos(th / 2)])


def _qmul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def _qrot(q, v):
    u = 2 * np.cross(q[:3], v)
    return v + q[3] * u + np.cross(q[:3], u)


def make_loop_trajectory(seed, n_kf=24, n_corrected=3, drift_rot=0.01, drift_trans=0.03, radius=5.0, scales=None,
                         loop_rot=0.0, loop_trans=0.0):
    """A synth_ba-style trajectory with one loop: n_kf key frames on a circle, odometry drift of drift_rot rad and
    drift_trans m per step, key frame n_kf - 1 closing on key frame 0.  The last n_corrected key frames carry corrected
    Sim3s (the drifted poses relative to the current key frame, moved onto its true pose; scales: their scales), all
    others (R, t, 1).  loop_rot / loop_trans: an extra error (rad, m, random direction) of the pose the loop puts the
    current key frame on.  returns dict(Scw, Scw_prior (SIM3_DTYPE[n_kf]), parent, cur_kf, loop_kf)."""
    rng = np.random.default_rng(seed)
    q_true, t_true = [], []
    for k in range(n_kf):
        a = 2 * math.pi * k / n_kf
        qwc = _quat_from_rotvec(np.array([0.0, 0.0, a]))
        pwc = np.array([radius * math.cos(a), radius * math.sin(a), 0.1 * math.sin(3 * a)])
        qcw = qwc * np.array([-1, -1, -1, 1.0])
        q_true.append(qcw), t_true.append(-_qrot(qcw, pwc))
    # drifted chain: T_k = (true relative motion, perturbed) * T_{k-1}
    q_d, t_d = [q_true[0]], [t_true[0]]
    for k in range(1, n_kf):
        q_prev_inv = q_true[k - 1] * np.array([-1, -1, -1, 1.0])
        q_rel = _qmul(q_true[k], q_prev_inv)
        t_rel = t_true[k] - _qrot(q_rel, t_true[k - 1])
        q_rel = _qmul(_quat_from_rotvec(rng.standard_normal(3) * drift_rot), q_rel)
        t_rel = t_rel + rng.standard_normal(3) * drift_trans
        q_d.append(_qmul(q_rel, q_d[-1])), t_d.append(_qrot(q_rel, t_d[-1]) + t_rel)
    prior = sim3_array(np.array(q_d), np.array(t_d))
    Scw = prior.copy()
    cur = n_kf - 1
    scales = [1.0] * n_corrected if scales is None else list(scales)
    q_cur_inv = q_d[cur] * np.array([-1, -1, -1, 1.0])
    axis, way = rng.standard_normal(3), rng.standard_normal(3)
    q_on = _qmul(_quat_from_rotvec(axis / np.linalg.norm(axis) * loop_rot), q_true[cur])
    t_on = t_true[cur] + way / np.linalg.norm(way) * loop_trans
    for c, k in enumerate(range(n_kf - n_corrected, n_kf)):
        # S_k,cur (drifted) * S_cur (true), with the scale of the correction
        q_rel = _qmul(q_d[k], q_cur_inv)
        t_rel = t_d[k] - _qrot(q_rel, t_d[cur])
        s = scales[c]
        Scw["q"][k] = _qmul(q_rel, q_on)
        Scw["t"][k] = _qrot(q_rel, t_on) + t_rel
        Scw["s"][k] = s
        Scw["t"][k] *= s
    parent = np.arange(-1, n_kf - 1)
    return dict(Scw=Scw, Scw_prior=prior, parent=parent, cur_kf=cur, loop_kf=0)
