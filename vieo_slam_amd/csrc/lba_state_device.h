// lba_state_device.h -- the state steps of the bundle-adjustment engine (lba.hip): what opens an optimize(), evaluates a
// state, moves the points and takes a rejected trial back.  Grids are (x, windows) x 256 threads unless said otherwise;
// ge / gq / gr = blocks of 256 edges / 64 points / max(256 points, 256 key frames) of the largest window.  All launched
// by launch_round (lba.hip), each under the control-word flag its first lines test.
//   k_lba_restore / k_lba_classify  rejected-step rollback (gr); chi2 / depth gates (ge): level (LBA_CLASS0) or erase
//   k_lba_prelevel   (ge), phases 0..2: the transform table at the call's states, Chi2LargeSetLevel, the far-point rule
//   k_lba_zero       (64): tab = -1 and the zero block CB[n_obs]
//   k_lba_begin      initializeOptimization(): active key frames / points from the edge levels, the
//                    reduced-system column of every free key frame, the (free kf, point) -> edge table; (windows) x 1024
//   k_lba_error      edge-parallel residuals + robust chi2 (per-block partial sums); (ge), LDS 32 B
//   k_lba_reduce     the partials -> the window's WinOut (or red_sc, sharded); (windows) x 256, LDS 96 B
//   k_lba_update_points  back-substitution x_l = D^-1 (b_l - B^T x_p), point update (with backup); (gq), LDS 32 B
//   k_lba_tail       the tail of a trial in one launch for calls of a few windows: the points, their edges' chi2, the pair
//                    edges (lba_generic_dev, mode 1), the fold; (gq + pairs), LDS 100 B + the pair edge's
// Reads   obs, level, ocam, cam / cams, close, the gates (thMono .. th_dist_far, dMono, dStereo), imu, kf_edge_first,
//         mp_first, mp_count, Hll, bl, CB, Bs, xp, gchi0, gchi, red.
// Writes  kf (col; restore), kf_list, np, n_free, npv, n_chunks, chunk_first / chunk_kf / chunk_cnt, kf_act, tab, mp_act,
//         xf, X, X_bak, scl[0] (restore), err, level, erase, part0, part, part_m, part_t, tail_cnt, red_sc, CB[n_obs].
#pragma once
#include "lba_inertial_device.h"

namespace vieo {

// ---- rollback of a rejected trial (g2o pop()): only what the trial changed
__global__ void __launch_bounds__(256)
k_lba_restore(const LbaDev* __restrict__ devs, const WinCtl* __restrict__ ctl) {
  const int w = blockIdx.y;
  if (!(ctl[w].flags & LBA_RESTORE)) return;
  const LbaDev& D = devs[w];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < D.n_mp && D.mp_act[i])
    for (int a = 0; a < 3; a++) D.X[3 * (size_t)i + a] = D.X_bak[3 * (size_t)i + a];
  if (i < D.n_kf && D.kf[i].col >= 0) {
    D.kf[i] = D.kf_bak[i];
    write_kf_xf(D, i, D.kf_bak[i]);
  }
  if (i == 0 && D.scale_opt) D.scl[0] = D.scl[1];
}

// chi2 (from the STORED error, as the reference does) / depth classification
// (Optimizer.cc:2191-2212 -> level 1; :2227-2249 -> vToErase)
__global__ void __launch_bounds__(256)
k_lba_classify(const LbaDev* __restrict__ devs, const WinCtl* __restrict__ ctl) {
  const int w = blockIdx.y, fl = ctl[w].flags;
  if (!(fl & (LBA_CLASS0 | LBA_CLASS1))) return;
  const LbaDev& D = devs[w];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= D.n_obs) return;
  const vieo_lba_obs o = D.obs[i];
  const double info = (double)o.inv_sigma2;
  const double* e = D.err + 3 * (size_t)i;
  double chi2 = e[0] * (info * e[0]) + e[1] * (info * e[1]);
  if (o.ur >= 0) chi2 += e[2] * (info * e[2]);
  const PoseXf& X = obs_xf(D, i, o.kf);  // (row 2 only)
  double Xw[3];
  scaled_point(D, o.mp, Xw);
  const double z = X.Rcw[6] * Xw[0] + X.Rcw[7] * Xw[1] + X.Rcw[8] * Xw[2] + X.tcw[2];
  const double th = o.ur >= 0 ? D.thStereo : ((D.close && D.close[o.mp]) ? D.thMonoClose : D.thMono);
  const bool bad = chi2 > th || !(z > 0.);
  if (fl & LBA_CLASS0) {
    if (bad) D.level[i] = 1;
  } else
    D.erase[i] = bad ? 1 : 0;
}

// GraphOperator::Chi2LargeSetLevel(edges, dim, 100.f, false) (g2o_graph_operator.h:23-40): every edge's
// error is computed and stored; chi2 > 100 * chi2_95(dim) puts the edge on level 1
__global__ void __launch_bounds__(256)
k_lba_prelevel(const LbaDev* __restrict__ devs, const WinCtl* __restrict__ ctl, int phase) {
  // phase 0: the transform table at the states the call came with (this is the first launch of such a window), and
  // clear the per-point marks (mp_act is free until k_lba_begin); phase 1: Chi2LargeSetLevel, and mark the
  // points a monocular edge sees closer than th_dist_far; phase 2: th_dist_far (Optimizer.cc:395,454,513-517) --
  // the monocular edges of an unmarked point go to level 1
  const int w = blockIdx.y;
  if (!(ctl[w].flags & LBA_PRELEVEL)) return;
  const LbaDev& D = devs[w];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool far_rule = D.th_dist_far > 0;
  if (phase == 0) {
    for (int k = i; k < D.n_kf; k += gridDim.x * 256) write_kf_xf(D, k, D.kf[k]);
    if (far_rule)
      for (int m = i; m < D.n_mp; m += gridDim.x * 256) D.mp_act[m] = 0;
    return;
  }
  if (i >= D.n_obs) return;
  const vieo_lba_obs o = D.obs[i];
  if (phase == 2) {
    if (far_rule && o.ur < 0 && !D.mp_act[o.mp]) D.level[i] = 1;
    return;
  }
  const CamD& C = obs_cam(D, i);
  const PoseXf& X = obs_xf(D, i, o.kf);
  double err[3], Pc[3], Xs[3];
  scaled_point(D, o.mp, Xs);
  const double chi2 = lba_edge_error(C, X, o, Xs, err, Pc);
  D.err[3 * (size_t)i] = err[0], D.err[3 * (size_t)i + 1] = err[1], D.err[3 * (size_t)i + 2] = err[2];
  if (far_rule && o.ur < 0 && Pc[2] < D.th_dist_far) D.mp_act[o.mp] = 1;  // same value from every writer
  const float th = 100.f * (o.ur >= 0 ? 7.815f : 5.991f);
  if (chi2 > (double)th) D.level[i] = 1;
}

// tab = -1 (and the zero block of CB) for the windows that start an optimize()
__global__ void __launch_bounds__(256)
k_lba_zero(const LbaDev* __restrict__ devs, const WinCtl* __restrict__ ctl) {
  const int w = blockIdx.y;
  if (!(ctl[w].flags & LBA_BEGIN)) return;
  const LbaDev& D = devs[w];
  const size_t nt = (size_t)D.nf_cap * D.n_mp;
  const size_t step = (size_t)gridDim.x * 256;
  if (blockIdx.x == 0 && threadIdx.x < 18) D.CB[18 * (size_t)D.n_obs + threadIdx.x] = 0.0;  // the zero block of absent pairs
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nt; i += step) D.tab[i] = -1;
}

// ---- initializeOptimization(0): one workgroup per window
__global__ void __launch_bounds__(1024)
k_lba_begin(LbaDev* __restrict__ devs, const WinCtl* __restrict__ ctl, WinOut* __restrict__ out) {
  const int w = blockIdx.x, tid = threadIdx.x;
  if (!(ctl[w].flags & LBA_BEGIN)) return;
  LbaDev& D = devs[w];
  const int n_mp = D.n_mp, n_obs = D.n_obs, n_kf = D.n_kf;
  int* s_act = D.kf_act;
  for (int k = tid; k < n_kf; k += 1024) {
    s_act[k] = 0;
    write_kf_xf(D, k, D.kf[k]);  // fixed key frames too: their entries are written here (or by k_lba_prelevel) only
  }
  for (int m = tid; m < n_mp; m += 1024) D.mp_act[m] = 0;
  __syncthreads();
  for (int i = tid; i < n_obs; i += 1024)
    if (D.level[i] == 0) {
      const vieo_lba_obs o = D.obs[i];
      s_act[o.kf] = 1;
      D.mp_act[o.mp] = 1;
    }
  if (D.pd == 6)  // encoder edges of a vision-only window are active edges too (their vertices join the system)
    for (int e = tid; e < D.n_imu; e += 1024) s_act[D.imu[e].i] = 1, s_act[D.imu[e].j] = 1;
  __syncthreads();
  if (tid == 0) {
    // vision-only window: free key frames with an active edge; visual-inertial window: the inertial
    // edges keep every free key frame active
    int np = 0, nf = 0;
    const int pd = D.pd;
    for (int k = 0; k < n_kf; k++) {
      if (!D.kf[k].fixed && (s_act[k] || pd == 15)) {
        D.kf[k].col = np, np += pd;
        D.kf_list[nf++] = k;
      } else
        D.kf[k].col = -1;
    }
    if (D.scale_opt) np += 1;  // id_scale = maxKFid + 1: after every key-frame vertex
    D.np = np, D.n_free = nf, D.npv = 6 * nf + (D.scale_opt ? 1 : 0);
    out[w].np = np;
    *D.tail_cnt = 0;  // (scratch memory: k_lba_tail's arrival counter starts an optimize() at zero)
    int nchk = 0;
    for (int a = 0; a < nf; a++) {
      const int k = D.kf_list[a];
      D.chunk_first[a] = nchk, D.chunk_cnt[a] = 0;
      nchk += max(1, (D.kf_edge_first[k + 1] - D.kf_edge_first[k] + kBuildChunk - 1) / kBuildChunk);
    }
    D.chunk_first[nf] = nchk, D.n_chunks = nchk;
  }
  __syncthreads();
  for (int a = tid; a < D.n_free; a += 1024)
    for (int c = D.chunk_first[a]; c < D.chunk_first[a + 1]; c++) D.chunk_kf[c] = a;
  for (int i = tid; i < n_obs; i += 1024)
    if (D.level[i] == 0) {
      const vieo_lba_obs o = D.obs[i];
      const int c = D.kf[o.kf].col;
      if (c >= 0) D.tab[(size_t)(c / D.pd) * n_mp + o.mp] = i;
    }
}

// ---- residuals + robust chi2 of the active edges.  which = 0: at the start of an optimize()
// (computeActiveErrors before the first iteration), which = 1: after a trial step
__global__ void __launch_bounds__(256)
k_lba_error(const LbaDev* __restrict__ devs, const WinCtl* __restrict__ ctl, int which) {
  __shared__ double s_red[4];
  const int w = blockIdx.y, fl = ctl[w].flags;
  if (!(fl & (which ? LBA_TRIAL : LBA_BEGIN))) return;
  const LbaDev& D = devs[w];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (blockIdx.x * 256 >= D.n_obs || D.np == 0) return;  // np == 0: optimize() returns before any error pass
  double v[1] = {0};
  if (i < D.n_obs && D.level[i] == 0) {
    const vieo_lba_obs o = D.obs[i];
    const CamD& C = obs_cam(D, i);
    const PoseXf& X = obs_xf(D, i, o.kf);
    double err[3], Pc[3], Xs[3];
    scaled_point(D, o.mp, Xs);
    const double chi2 = lba_edge_error(C, X, o, Xs, err, Pc);
    D.err[3 * (size_t)i] = err[0], D.err[3 * (size_t)i + 1] = err[1], D.err[3 * (size_t)i + 2] = err[2];
    double r0 = chi2, r1;
    if (fl & LBA_ROBUST) {
      const double dl = o.ur >= 0 ? D.dStereo : D.dMono;
      huber(chi2, dl, dl * dl, &r0, &r1);
    }
    v[0] = r0;
  }
  block_sum<1>(v, s_red, threadIdx.x);
  if (threadIdx.x == 0) (which ? D.part : D.part0)[blockIdx.x] = v[0];
}

// one workgroup per window: fold the per-block partials into the window's output record
// per_point: the trial's chi2 partials are k_lba_tail's (one per block of 64 points) instead of k_lba_error's
__device__ __forceinline__ void lba_reduce_dev(const LbaDev& D, const WinCtl* __restrict__ ctl, WinOut* __restrict__ out, int w,
                                               int fl, bool per_point, double* s_red) {
  double v[3] = {0, 0, 0};
  if ((fl & LBA_BEGIN) && D.np > 0)
    for (int i = threadIdx.x; i < (D.n_obs + 255) / 256; i += 256) v[0] += D.part0[i];
  if ((fl & LBA_TRIAL) && D.np > 0) {
    if (per_point)
      for (int i = threadIdx.x; i < (D.n_mp + 63) / 64; i += 256) v[1] += D.part_t[i];
    else
      for (int i = threadIdx.x; i < (D.n_obs + 255) / 256; i += 256) v[1] += D.part[i];
    for (int i = threadIdx.x; i < (D.n_mp + 63) / 64; i += 256) v[2] += D.part_m[i];
  }
  block_sum<3>(v, s_red, threadIdx.x);
  if (threadIdx.x == 0) {
    double g0 = 0, g1 = 0;  // inertial edges, fixed order
    for (int e = 0; e < D.n_imu; e++) g0 += D.gchi0[e], g1 += D.gchi[e];
    if (D.red) {  // visual parts go through the all-reduce, the inertial part is the same on every rank
      double* sc = D.red_sc;
      sc[0] = v[0], sc[1] = v[1], sc[2] = v[2];
      sc[3] = ctl[w].pad ? 1.0 : 0.0;  // this rank's stop request: summed with the others', every rank sees the same count
      out[w].chig0 = g0, out[w].chig = (fl & LBA_TRIAL) ? g1 : 0.0;
    } else
      out[w].chi0 = v[0] + g0, out[w].chi2 = v[1] + ((fl & LBA_TRIAL) ? g1 : 0.0), out[w].scale_l = v[2];
  }
}
__global__ void __launch_bounds__(256)
k_lba_reduce(const LbaDev* __restrict__ devs, const WinCtl* __restrict__ ctl, WinOut* __restrict__ out) {
  __shared__ double s_red[4 * 3];
  const int w = blockIdx.x, fl = ctl[w].flags;
  if (!(fl & (LBA_TRIAL | LBA_BEGIN))) return;
  lba_reduce_dev(devs[w], ctl, out, w, fl, false, s_red);
}

// ---- back-substitution + update of the points, landmark part of the LM gain-ratio scale
// (the body: k_lba_update_points, and k_lba_tail which goes on with the points' edges)
// Xn (optional): the updated point on the quad's lane 0, zeros on the other lanes and for an inactive point
__device__ __forceinline__ void lba_update_points_dev(const LbaDev& D, double lambda, int blk, double* s_red, double* Xn = nullptr) {
  // FOUR lanes per point, each over every fourth free key frame: a point's chain was one dependent `tab` -> block round
  // trip per free key frame (10 .. 25 of them, 73 us per launch whatever the batch); the quad's partial sums are added
  // in a fixed order
  const int m = blk * 64 + (threadIdx.x >> 2), sub = threadIdx.x & 3;
  const bool act = m < D.n_mp && D.mp_act[m];
  double sc[1] = {0};
  double cl[3] = {0, 0, 0};
  if (act) {
    if (sub == 0) cl[0] = D.bl[3 * (size_t)m], cl[1] = D.bl[3 * (size_t)m + 1], cl[2] = D.bl[3 * (size_t)m + 2];
    for (int a = sub; a < D.n_free; a += 4) {
      const int e = D.tab[(size_t)a * D.n_mp + m];
      if (e < 0) continue;
      const double* B = D.CB + 18 * (size_t)e;
      for (int r = 0; r < 6; r++, B += 3) {
        const double xa = D.xp[D.pd * a + r];
        cl[0] -= B[0] * xa, cl[1] -= B[1] * xa, cl[2] -= B[2] * xa;
      }
    }
    if (D.scale_opt && sub == 0) {  // the (scale, point) block
      const double* B = D.Bs + 3 * (size_t)m;
      const double xa = D.xp[D.np - 1];
      cl[0] -= B[0] * xa, cl[1] -= B[1] * xa, cl[2] -= B[2] * xa;
    }
  }
#pragma unroll
  for (int k = 0; k < 3; k++) cl[k] = quad_sum_f64(cl[k]);
  if (act && sub == 0) {
    double Di[9];
    landmark_dinv(D.Hll + 9 * (size_t)m, lambda, Di);
    for (int a = 0; a < 3; a++) {
      const double x = Di[a * 3] * cl[0] + Di[a * 3 + 1] * cl[1] + Di[a * 3 + 2] * cl[2];
      const double old = D.X[3 * (size_t)m + a];
      D.X_bak[3 * (size_t)m + a] = old;
      D.X[3 * (size_t)m + a] = old + x;
      if (Xn) Xn[a] = old + x;
      sc[0] += x * (lambda * x + D.bl[3 * (size_t)m + a]);
    }
  }
  block_sum<1>(sc, s_red, threadIdx.x);
  if (threadIdx.x == 0) D.part_m[blk] = sc[0];  // one partial per 64 points (k_lba_reduce)
}
__global__ void __launch_bounds__(256)
k_lba_update_points(const LbaDev* __restrict__ devs, const WinCtl* __restrict__ ctl,
                    const WinOut* __restrict__ out) {
  __shared__ double s_red[4];
  const int w = blockIdx.y;
  if (!(ctl[w].flags & LBA_TRIAL)) return;
  const LbaDev& D = devs[w];
  if (blockIdx.x * 64 >= D.n_mp || D.np == 0) return;
  lba_update_points_dev(D, win_lambda(ctl[w], out[w]), blockIdx.x, s_red);
}

// ---- the tail of a trial as ONE launch (round 6; were k_lba_update_points, k_lba_error(1), k_lba_generic(1),
// k_lba_reduce: four dependent launches of 5-6 us each that are mostly launch ramp).
//   workgroups [0, gq): 64 points each -- back-substitution and update of the points as above, then the residuals and the
//     robust chi2 of THOSE points' edges (a point's observations are contiguous; the quad of a point takes every fourth;
//     the key-frame poses were updated by the solve kernel before this launch): no workgroup waits for another;
//   workgroups [gq, gq + pairs): the inertial / encoder pair edges' chi2 after the trial (one wavefront each);
//   the LAST workgroup of a window to arrive (a counter in global memory behind a device-scope fence) folds the
//     partials into the window's output record in k_lba_reduce's fixed order.
// Calls of a few windows only (D.fold_kernel == 0); batches take the four launches.
// The trial's visual chi2 is summed per block of 64 points instead of per block of 256 edges: another (fixed)
// association order than the four-launch form, same terms.
__global__ void __launch_bounds__(256)
k_lba_tail(const LbaDev* __restrict__ devs, const WinCtl* __restrict__ ctl, WinOut* __restrict__ out, int gq) {
  __shared__ double s_red[4 * 3];
  __shared__ int s_last;
  const int w = blockIdx.y, fl = ctl[w].flags;
  if (!(fl & LBA_TRIAL)) return;
  const LbaDev& D = devs[w];
  const int nblk = max((D.n_mp + 63) / 64, 1);  // (block 0 of an empty landmark shard still arrives)
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < gq) {
    if ((int)blockIdx.x >= nblk) return;
    if (D.np > 0 && (int)blockIdx.x * 64 < D.n_mp) {
      double Xn[3] = {0, 0, 0};
      lba_update_points_dev(D, win_lambda(ctl[w], out[w]), blockIdx.x, s_red, Xn);
      // the edges of the block's points at the trial state (the new point travels from the quad's lane 0 in registers:
      // x + 0 + 0 + 0 is exact)
      const int m = blockIdx.x * 64 + (tid >> 2), sub = tid & 3;
#pragma unroll
      for (int a = 0; a < 3; a++) Xn[a] = quad_sum_f64(Xn[a]);
      double v[1] = {0};
      if (m < D.n_mp && D.mp_act[m]) {  // (a point without an active edge has nothing to evaluate)
        const int first = D.mp_first[m], cnt = D.mp_count[m];
        const double scl = win_scale(D);
        const double Xs[3] = {Xn[0] * scl, Xn[1] * scl, Xn[2] * scl};
        for (int k = sub; k < cnt; k += 4) {
          const int i = first + k;
          if (D.level[i] != 0) continue;
          const vieo_lba_obs o = D.obs[i];
          const CamD& C = obs_cam(D, i);
          const PoseXf& X = obs_xf(D, i, o.kf);
          double err[3], Pc[3];
          const double chi2 = lba_edge_error(C, X, o, Xs, err, Pc);
          D.err[3 * (size_t)i] = err[0], D.err[3 * (size_t)i + 1] = err[1], D.err[3 * (size_t)i + 2] = err[2];
          double r0 = chi2, r1;
          if (fl & LBA_ROBUST) {
            const double dl = o.ur >= 0 ? D.dStereo : D.dMono;
            huber(chi2, dl, dl * dl, &r0, &r1);
          }
          v[0] += r0;
        }
      }
      v[0] = quad_sum_f64(v[0]);
      if (sub != 0) v[0] = 0;
      block_sum<1>(v, s_red, tid);
      if (tid == 0) D.part_t[blockIdx.x] = v[0];
    }
  } else {
    const int e = blockIdx.x - gq;
    if (e >= D.n_imu) return;
    if (tid < 64) lba_generic_dev(D, e, tid, 1);
  }
  // arrival: this workgroup's results are visible device-wide before its count is
  __threadfence();
  __syncthreads();
  if (tid == 0) {
    const int total = nblk + D.n_imu;
    const int old = atomicAdd(D.tail_cnt, 1);
    s_last = old == total - 1;
    if (s_last) *D.tail_cnt = 0;  // (for the next launch: nobody else touches it any more)
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  lba_reduce_dev(D, ctl, out, w, fl, true, s_red);
}

}  // namespace vieo
