// lba_linearize_device.h -- linearisation of the visual edges of the bundle-adjustment engine (lba.hip): buildSystem
// (block_solver.hpp:451-520) and computeLambdaInit.  Grids are (x, windows); launched by launch_round (lba.hip),
// k_lba_build and its folds under LBA_BUILD, k_lba_lambda under LBA_BEGIN.
//   k_lba_build<MULTICAM, SCALE, HALF>  buildSystem: four lanes per point over its observations (H_ll, b_l); one
//                    workgroup per run of a free key frame's edge list (H_pp, b_p) which also writes the
//                    6 x 3 blocks B = Jp^T W Jx of its edges, COMPACT: one 144-byte block per observation
//                    (CB[edge]); `tab` maps (free key frame, point) to the edge that carries the block.
//                    256 threads, LDS 864 B + the arrival flag; HALF 0: gq blocks of 64 points, 1: the windows' chunks, 2 (calls of a few
//                    windows): both and the pair edges behind them (lba_generic_dev, mode 0: + its LDS)
//   k_lba_build_fold  (free key frames) x 64: a key frame's runs added in run order (batches, fold_kernel)
//   k_lba_scale_fold  (windows) x 256, LDS 64 B: H_ss, b_s of the scale vertex from the point half's partials
//   k_lba_lambda     computeLambdaInit (tau * max diagonal) for windows starting an optimize(); (windows) x 256, LDS 2 KB
// Reads   obs, level, ocam, cam / cams, xf, kf, X, scl, mp_act, mp_first, mp_count, kf_edge_first, kf_edge_idx, kf_list,
//         tab, chunk_first, chunk_kf, n_chunks, fold_kernel, dMono, dStereo; k_lba_lambda also kf_in, kf_out, Ae.
// Writes  Hll, bl, pmax, Bs, psc (point half); CB, Hpp, bp, sc_sys, chunk_part, chunk_cnt (key-frame half and the
//         folds); out[w].lambda (k_lba_lambda).
#pragma once
#include "lba_inertial_device.h"

namespace vieo {

// 6x3 block Jp^T (rho' Omega) Jx of one active edge (multi-camera rigs: a key frame can see a point in
// several cameras, the (key frame, point) block of BB is the sum over those edges)
__device__ __forceinline__ void lba_edge_B(const LbaDev& D, int i, const LbaKf& k, bool robust, double* B) {
  const vieo_lba_obs o = D.obs[i];
  const CamD& C = obs_cam(D, i);
  const PoseXf& X = obs_xf(D, i, o.kf);
  double Xw[3];
  scaled_point(D, o.mp, Xw);
  const double sc = win_scale(D);
  double err[3], Pc[3];
  const double chi2 = lba_edge_error(C, X, o, Xw, err, Pc);
  const bool stereo = o.ur >= 0;
  double r0, r1 = 1.;
  if (robust) {
    const double dl = stereo ? D.dStereo : D.dMono;
    huber(chi2, dl, dl * dl, &r0, &r1);
  }
  double Jp[18], Jx[9];
  lba_jacobians(C, X, k.p, Xw, Pc, Jp, Jx);
  const double ww = r1 * (double)o.inv_sigma2;
  if (!stereo) Jx[6] = Jx[7] = Jx[8] = 0;
  if (D.scale_opt)
    for (int t = 0; t < 9; t++) Jx[t] *= sc;  // J_Xh = s (Jproj Rcw)
#pragma unroll
  for (int q = 0; q < 6; q++)
#pragma unroll
    for (int b = 0; b < 3; b++) B[q * 3 + b] = Jp[q] * ww * Jx[b] + Jp[6 + q] * ww * Jx[3 + b] + Jp[12 + q] * ww * Jx[6 + b];
}

// ---- buildSystem (block_solver.hpp:451-520 with EdgeReprojectPR[Stereo]::linearizeOplus).
// blocks [0, gm): four lanes per point over its (contiguous) observations -> H_ll, b_l;
// blocks [gm, gm + free key frames): one workgroup per key frame over its edge list -> H_pp, b_p and the
// rows of BB = Jp^T W Jx it owns.  Every sum has a fixed order.
// MULTICAM: windows with several (distorted) cameras per key frame; the single rectified camera keeps the
// lean instantiation.  SCALE: a batch with a scale-vertex window (EdgeReprojectPRS[Stereo]): the point half also forms
// the point's entry of the scale row of BB (sum over its edges of Js^T W Jx) and its terms of H_ss / b_s, the key-frame
// half H_ps = sum Jp^T W Js.
// The two halves are two launches (KFHALF): the point half is held to 168 registers (its launch bound: three wavefronts
// per SIMD; 188 without the bound, 212 while it derived the transforms itself from four poses loaded ahead), the key-frame
// half takes all 256, and in one kernel the point half's 64 % of the workgroups ran at the key-frame half's two
// wavefronts per SIMD.
// The key-frame half takes a key frame's edge list in chunks of kBuildChunk edges, one workgroup per chunk (a rig key
// frame has thousands of edges -- 4 cameras x 1500 features: one workgroup per key frame was 1.08 ms of a trial's 1.4);
// a chunk's sums go to chunk_part, the workgroup that arrives last at the key frame's counter adds the chunks in chunk
// order.  A key frame of one chunk (<= kBuildChunk edges) writes its sums directly, as before.
// The one-launch instance (HALF = 2, calls of a few windows) also carries the generic (inertial / encoder) edges'
// linearisation, one workgroup per edge behind the gk chunk workgroups (k_lba_generic(0) otherwise: 44 us of single-lane
// chains that then run beside the chunks instead of behind them).
// HALF = 0: the point half, 1: the key-frame half (+ the generic edges), 2: both in one launch -- gp point workgroups, then
// the key-frame half's (calls of a few windows: the register-rich instance's occupancy does not matter there, a launch
// less does).
template <bool MULTICAM, bool SCALE, int HALF>
__global__ void __launch_bounds__(256, HALF == 0 ? 3 : 2)
k_lba_build(const LbaDev* __restrict__ devs, const WinCtl* __restrict__ ctl, int gk, int gp) {
  int bx = blockIdx.x;
  __shared__ double s_red[4 * 27];
  const int w = blockIdx.y, fl = ctl[w].flags;
  if (!(fl & LBA_BUILD)) return;
  const LbaDev& D = devs[w];
  const bool point_half = HALF == 0 || (HALF == 2 && bx < gp);
  if (HALF == 2 && !point_half) bx -= gp;
  if (HALF == 2 && !point_half && bx >= gk) {  // (this instance only: the generic path's 1.7 KB of scratch per lane would
    const int e = bx - gk;                     //  cost the batched key-frame half its occupancy: 3.2 -> 15.6 ms per step)
    if (e < D.n_imu && threadIdx.x < 64) lba_generic_dev(D, e, threadIdx.x, 0);
    return;
  }
  if (D.np == 0) return;
  const bool robust = fl & LBA_ROBUST;
  if (point_half) {
    if (bx * 64 >= D.n_mp) return;
    const int m = bx * 64 + (threadIdx.x >> 2), sub = threadIdx.x & 3;  // 4 lanes per point
    const bool act = m < D.n_mp && D.mp_act[m];
    double mx = 0;
    double acc[9];
#pragma unroll
    for (int t = 0; t < 9; t++) acc[t] = 0;
    double asc[5] = {0, 0, 0, 0, 0};  // SCALE: Bs[3], H_ss, b_s of the point
    const bool scl = SCALE && D.scale_opt;
    const double sc = scl ? D.scl[0] : 1.0;
    if (act) {
      const double Xh[3] = {D.X[3 * (size_t)m], D.X[3 * (size_t)m + 1], D.X[3 * (size_t)m + 2]};
      const double Xw[3] = {Xh[0] * sc, Xh[1] * sc, Xh[2] * sc};
      const int first = D.mp_first[m], cnt = D.mp_count[m];
      // A lane's edges four at a time: their records and level bytes first, then the arithmetic, each edge on its key
      // frame's entry of the transform table (Rcw, tcw: twelve loads off the record, nothing to derive) -- the records'
      // two dependent round trips per FOUR edges instead of per edge.  Same edges in the same order per lane, so the
      // sums are bit-identical.
      for (int j0 = sub; j0 < cnt; j0 += 16) {
        vieo_lba_obs ou[4];
        unsigned char lv[4], oc[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const int i = first + min(j0 + 4 * u, cnt - 1);
          ou[u] = D.obs[i], lv[u] = D.level[i];
          oc[u] = (MULTICAM && D.n_cams) ? D.ocam[i] : (unsigned char)0;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
        if (j0 + 4 * u >= cnt || lv[u]) continue;
        const vieo_lba_obs o = ou[u];
        const CamD& C = (MULTICAM && D.n_cams) ? D.cams[oc[u]] : D.cam;
        const PoseXf& X = D.xf[(MULTICAM && D.n_cams) ? (size_t)o.kf * D.n_cams + oc[u] : (size_t)o.kf];
        double err[3], Pc[3];
        const double chi2 = lba_edge_error(C, X, o, Xw, err, Pc);
        const bool stereo = o.ur >= 0;
        double r0, r1 = 1.;
        if (robust) {
          const double dl = stereo ? D.dStereo : D.dMono;
          huber(chi2, dl, dl * dl, &r0, &r1);
        }
        const double invz = 1 / Pc[2], invz2 = invz * invz;
        double J[9], Jx[9], Jc[6], uv[2];
        cam_project(C, Pc, uv, Jc);
        J[0] = -Jc[0], J[1] = -Jc[1], J[2] = -Jc[2];
        J[3] = -Jc[3], J[4] = -Jc[4], J[5] = -Jc[5];
        J[6] = J[0], J[7] = J[1], J[8] = J[2] - C.bf * invz2;
        for (int r = 0; r < 3; r++)
          for (int q = 0; q < 3; q++)
            Jx[r * 3 + q] = J[r * 3] * X.Rcw[q] + J[r * 3 + 1] * X.Rcw[3 + q] + J[r * 3 + 2] * X.Rcw[6 + q];
        const double info = (double)o.inv_sigma2, ww = r1 * info;
        if (!stereo) Jx[6] = Jx[7] = Jx[8] = 0;  // monocular edge: no third row (err[2] is 0 already)
        if (scl) {  // _jacobianOplus[scale] = _jacobianOplus[0] * Ph_unscale, then _jacobianOplus[0] *= scale
          double Js[3];
#pragma unroll
          for (int r = 0; r < 3; r++) Js[r] = Jx[r * 3] * Xh[0] + Jx[r * 3 + 1] * Xh[1] + Jx[r * 3 + 2] * Xh[2];
#pragma unroll
          for (int q = 0; q < 9; q++) Jx[q] *= sc;
#pragma unroll
          for (int b = 0; b < 3; b++) asc[b] += Js[0] * ww * Jx[b] + Js[1] * ww * Jx[3 + b] + Js[2] * ww * Jx[6 + b];
          asc[3] += Js[0] * ww * Js[0] + Js[1] * ww * Js[1] + Js[2] * ww * Js[2];
          asc[4] += Js[0] * (-(info * err[0]) * r1) + Js[1] * (-(info * err[1]) * r1) + Js[2] * (-(info * err[2]) * r1);
        }
        int t = 0;
#pragma unroll
        for (int a = 0; a < 3; a++) {
#pragma unroll
          for (int b = a; b < 3; b++, t++)
            acc[t] += Jx[a] * ww * Jx[b] + Jx[3 + a] * ww * Jx[3 + b] + Jx[6 + a] * ww * Jx[6 + b];
          acc[6 + a] += Jx[a] * (-(info * err[0]) * r1) + Jx[3 + a] * (-(info * err[1]) * r1) +
                        Jx[6 + a] * (-(info * err[2]) * r1);
        }
        }
      }
    }
#pragma unroll
    for (int t = 0; t < 9; t++) acc[t] = quad_sum_f64(acc[t]);
    if (act && sub == 0) {
      double* H = D.Hll + 9 * (size_t)m;
      H[0] = acc[0], H[1] = acc[1], H[2] = acc[2];
      H[3] = acc[1], H[4] = acc[3], H[5] = acc[4];
      H[6] = acc[2], H[7] = acc[4], H[8] = acc[5];
      D.bl[3 * (size_t)m] = acc[6], D.bl[3 * (size_t)m + 1] = acc[7], D.bl[3 * (size_t)m + 2] = acc[8];
      mx = fmax(fabs(acc[0]), fmax(fabs(acc[3]), fabs(acc[5])));
    }
    if (scl) {
#pragma unroll
      for (int t = 0; t < 5; t++) asc[t] = quad_sum_f64(asc[t]);
      if (m < D.n_mp && sub == 0) {  // the scale's row of BB: zero for a point without an active edge
        double* B = D.Bs + 3 * (size_t)m;
        B[0] = asc[0], B[1] = asc[1], B[2] = asc[2];
      }
      double v[2] = {sub == 0 ? asc[3] : 0.0, sub == 0 ? asc[4] : 0.0};
      block_sum<2>(v, s_red + 8, threadIdx.x);
      if (threadIdx.x == 0) D.psc[2 * bx] = v[0], D.psc[2 * bx + 1] = v[1];
    }
    // landmark part of computeLambdaInit: block maximum
    mx = wave_max_f64(mx);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) D.pmax[bx] = fmax(fmax(s_red[0], s_red[1]), fmax(s_red[2], s_red[3]));
    return;
  }
  if (bx >= D.n_chunks) return;
  const int a = D.chunk_kf[bx], chunk0 = D.chunk_first[a], nchunk = D.chunk_first[a + 1] - chunk0;
  const int kfi = D.kf_list[a];
  const LbaKf k = D.kf[kfi];
  const int first = D.kf_edge_first[kfi], cnt = D.kf_edge_first[kfi + 1] - first;
  // The sums are formed per run of kBuildChunk edges (a workgroup each) and the runs' sums added in run order: by the last
  // workgroup of the key frame to arrive in calls of a few windows, by k_lba_build_fold in batches (D.fold_kernel: a
  // device-scope fence per workgroup does not scale) -- the same association either way, a window's result does not depend
  // on what it is batched with.
  const int j_lo = (bx - chunk0) * kBuildChunk, j_hi = min(cnt, j_lo + kBuildChunk);
  double acc[27];
  double aps[6] = {0, 0, 0, 0, 0, 0};  // SCALE: H_ps = sum Jp^T W Js
#pragma unroll
  for (int t = 0; t < 27; t++) acc[t] = 0;
  const bool scl = SCALE && D.scale_opt;
  const double sc = scl ? D.scl[0] : 1.0;
  PoseXf X;
  if (!(MULTICAM && D.n_cams)) X = D.xf[kfi];  // one camera: the transform is the same for all edges of the key frame
  const int* tab_a = D.tab + (size_t)a * D.n_mp;
  // A thread's edges two at a time: both list entries, then both records and level bytes, then both points are loaded
  // before the arithmetic (three dependent round trips per PAIR of edges instead of per edge; a key frame's ~600 edges are
  // 2.3 per thread).  Same edges in the same order per thread: the sums are bit-identical.
  for (int j0 = j_lo + threadIdx.x; j0 < j_hi; j0 += 512) {  // (one trip: a run is 2 edges per thread)
    int ii[2];
    vieo_lba_obs oo[2];
    unsigned char lvv[2];
    double Xp[2][3];
#pragma unroll
    for (int u = 0; u < 2; u++) ii[u] = D.kf_edge_idx[first + min(j0 + 256 * u, cnt - 1)];
#pragma unroll
    for (int u = 0; u < 2; u++) oo[u] = D.obs[ii[u]], lvv[u] = D.level[ii[u]];
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const double* q = D.X + 3 * (size_t)oo[u].mp;
      Xp[u][0] = q[0], Xp[u][1] = q[1], Xp[u][2] = q[2];
    }
#pragma unroll
    for (int u = 0; u < 2; u++) {
    const int j = j0 + 256 * u;
    if (j >= j_hi) continue;
    const int i = ii[u];
    const vieo_lba_obs o = oo[u];
    const bool active = !lvv[u];
    double Bk[18];
#pragma unroll
    for (int t = 0; t < 18; t++) Bk[t] = 0;
    if (active) {
      const double* Xh = Xp[u];
      const double Xw[3] = {Xh[0] * sc, Xh[1] * sc, Xh[2] * sc};
      double err[3], Pc[3];
      const CamD& C = obs_cam(D, i);
      if (MULTICAM && D.n_cams) X = obs_xf(D, i, kfi);
      const double chi2 = lba_edge_error(C, X, o, Xw, err, Pc);
      const bool stereo = o.ur >= 0;
      double r0, r1 = 1.;
      if (robust) {
        const double dl = stereo ? D.dStereo : D.dMono;
        huber(chi2, dl, dl * dl, &r0, &r1);
      }
      double Jp[18], Jx[9];
      lba_jacobians(C, X, k.p, Xw, Pc, Jp, Jx);
      const double info = (double)o.inv_sigma2, ww = r1 * info;
      visual_accumulate(Jp, err, info, r1, stereo, acc);
      if (!stereo) Jx[6] = Jx[7] = Jx[8] = 0;
      if (scl) {
        double Js[3];
#pragma unroll
        for (int r = 0; r < 3; r++) Js[r] = Jx[r * 3] * Xh[0] + Jx[r * 3 + 1] * Xh[1] + Jx[r * 3 + 2] * Xh[2];
#pragma unroll
        for (int q = 0; q < 9; q++) Jx[q] *= sc;
#pragma unroll
        for (int q = 0; q < 6; q++) {
          double t = Jp[q] * ww * Js[0] + Jp[6 + q] * ww * Js[1];
          if (stereo) t += Jp[12 + q] * ww * Js[2];
          aps[q] += t;
        }
      }
#pragma unroll
      for (int q = 0; q < 6; q++)
#pragma unroll
        for (int b = 0; b < 3; b++)
          Bk[q * 3 + b] = Jp[q] * ww * Jx[b] + Jp[6 + q] * ww * Jx[3 + b] + Jp[12 + q] * ww * Jx[6 + b];
    }
    // the (key frame, point) block lives at the edge `tab` points to; with several cameras per key frame that edge
    // sums the run of the pair's edges (adjacent in the list) in list order
    bool write = active;
    if (MULTICAM && D.n_cams) {
      write = false;
      if (tab_a[o.mp] == i) {
        int js = j;
        while (js > 0 && D.obs[D.kf_edge_idx[first + js - 1]].mp == o.mp) js--;
        double Bsum[18];
#pragma unroll
        for (int t = 0; t < 18; t++) Bsum[t] = 0;
        bool first_term = true;
        for (int jj = js; jj < cnt; jj++) {
          const int i2 = D.kf_edge_idx[first + jj];
          if (D.obs[i2].mp != o.mp) break;
          if (D.level[i2]) continue;
          double B2[18];
          if (jj == j) {
#pragma unroll
            for (int t = 0; t < 18; t++) B2[t] = Bk[t];
          } else
            lba_edge_B(D, i2, k, robust, B2);
#pragma unroll
          for (int t = 0; t < 18; t++) Bsum[t] = first_term ? B2[t] : Bsum[t] + B2[t];
          first_term = false;
          write = true;
        }
#pragma unroll
        for (int t = 0; t < 18; t++) Bk[t] = Bsum[t];
      }
    }
    if (write) {
      double* B = D.CB + 18 * (size_t)i;
#pragma unroll
      for (int t = 0; t < 18; t++) B[t] = Bk[t];
    }
    }
  }
  block_sum<27>(acc, s_red, threadIdx.x);
  if (scl) block_sum<6>(aps, s_red, threadIdx.x);
  __shared__ int s_last;
  if (nchunk > 1) {  // this chunk's sums; the last workgroup of the key frame adds the chunks in order
    if (threadIdx.x < 33) {
      double v = 0;
#pragma unroll
      for (int t = 0; t < 27; t++)
        if ((int)threadIdx.x == t) v = acc[t];
#pragma unroll
      for (int t = 0; t < 6; t++)
        if ((int)threadIdx.x == 27 + t) v = aps[t];
      D.chunk_part[33 * (size_t)bx + threadIdx.x] = v;
    }
    if (D.fold_kernel) return;  // (batches: k_lba_build_fold adds the runs)
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) {
      const int old = atomicAdd(&D.chunk_cnt[a], 1);
      s_last = old == nchunk - 1;
      if (s_last) D.chunk_cnt[a] = 0;  // (for the next launch: nobody else touches it any more)
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    if (threadIdx.x < 33) {
      double v = 0;
      for (int c = 0; c < nchunk; c++) v += D.chunk_part[33 * (size_t)(chunk0 + c) + threadIdx.x];
#pragma unroll
      for (int t = 0; t < 27; t++)
        if ((int)threadIdx.x == t) acc[t] = v;
#pragma unroll
      for (int t = 0; t < 6; t++)
        if ((int)threadIdx.x == 27 + t) aps[t] = v;
    }
  }
  if (threadIdx.x < 27) {
    double v = 0;
#pragma unroll
    for (int t = 0; t < 27; t++)  // select, not acc[threadIdx.x]: keeps the sums in registers
      if ((int)threadIdx.x == t) v = acc[t];
    if (threadIdx.x < 21) {
      int r = 0, t = threadIdx.x;
      while (t >= 6 - r) t -= 6 - r, r++;
      const int c = r + t;
      D.Hpp[36 * (size_t)a + r * 6 + c] = v;
      D.Hpp[36 * (size_t)a + c * 6 + r] = v;
    } else
      D.bp[6 * a + threadIdx.x - 21] = v;
  }
  if (scl && threadIdx.x >= 27 && threadIdx.x < 33) {
    double v = 0;
#pragma unroll
    for (int t = 0; t < 6; t++)
      if ((int)threadIdx.x == 27 + t) v = aps[t];
    D.sc_sys[6 * a + threadIdx.x - 27] = v;
  }
}

// The runs' sums of a key frame added in run order (batches; see k_lba_build): one wavefront per free key frame
__global__ void __launch_bounds__(64)
k_lba_build_fold(const LbaDev* __restrict__ devs, const WinCtl* __restrict__ ctl) {
  const int w = blockIdx.y;
  if (!(ctl[w].flags & LBA_BUILD)) return;
  const LbaDev& D = devs[w];
  const int a = blockIdx.x;
  if (D.np == 0 || a >= D.n_free) return;
  const int chunk0 = D.chunk_first[a], nchunk = D.chunk_first[a + 1] - chunk0;
  if (nchunk <= 1 || threadIdx.x >= 33) return;
  double v = 0;
  for (int c = 0; c < nchunk; c++) v += D.chunk_part[33 * (size_t)(chunk0 + c) + threadIdx.x];
  if (threadIdx.x < 21) {
    int r = 0, t = threadIdx.x;
    while (t >= 6 - r) t -= 6 - r, r++;
    const int c = r + t;
    D.Hpp[36 * (size_t)a + r * 6 + c] = v;
    D.Hpp[36 * (size_t)a + c * 6 + r] = v;
  } else if (threadIdx.x < 27)
    D.bp[6 * a + threadIdx.x - 21] = v;
  else if (D.scale_opt)
    D.sc_sys[6 * a + threadIdx.x - 27] = v;
}

// H_ss, b_s of the scale vertex: the per-block partials of k_lba_build in fixed order (one workgroup per window)
__global__ void __launch_bounds__(256)
k_lba_scale_fold(const LbaDev* __restrict__ devs, const WinCtl* __restrict__ ctl) {
  __shared__ double s_red[4 * 2];
  const int w = blockIdx.x;
  if (!(ctl[w].flags & LBA_BUILD)) return;
  const LbaDev& D = devs[w];
  if (!D.scale_opt || D.np == 0) return;
  double v[2] = {0, 0};
  for (int i = threadIdx.x; i < (D.n_mp + 63) / 64; i += 256) v[0] += D.psc[2 * i], v[1] += D.psc[2 * i + 1];
  block_sum<2>(v, s_red, threadIdx.x);
  if (threadIdx.x == 0) D.sc_sys[6 * D.n_free] = v[0], D.sc_sys[6 * D.n_free + 1] = v[1];
}

// computeLambdaInit: tau * max |diagonal| over the pose and landmark blocks (one workgroup per window)
__global__ void __launch_bounds__(256)
k_lba_lambda(const LbaDev* __restrict__ devs, const WinCtl* __restrict__ ctl, WinOut* __restrict__ out) {
  __shared__ double s_m[256];
  const int w = blockIdx.x;
  if (!(ctl[w].flags & LBA_BEGIN)) return;
  const LbaDev& D = devs[w];
  double mx = 0;
  if (D.scale_opt && threadIdx.x == 0) mx = fabs(D.sc_sys[6 * D.n_free]);  // H_ss
  if (D.pd == 6 && D.n_imu == 0) {
    for (int j = threadIdx.x; j < 6 * D.n_free; j += 256) mx = fmax(mx, fabs(D.Hpp[36 * (size_t)(j / 6) + 7 * (j % 6)]));
  } else {  // PR + V + Bias vertices: visual block + the inertial edges' diagonal (as k_lba_assemble adds them)
    for (int j = threadIdx.x; j < D.pd * D.n_free; j += 256) {
      const int pd = D.pd, a = j / pd, ra = j - a * pd, ka = D.kf_list[a];
      const int ein = D.kf_in[ka], eout = D.kf_out[ka];
      double v = ra < 6 ? D.Hpp[36 * (size_t)a + 7 * ra] : 0.0;
      if (ein >= 0) v += D.Ae[930 * (size_t)ein + (15 + ra) * 30 + 15 + ra];
      if (eout >= 0) v += D.Ae[930 * (size_t)eout + ra * 30 + ra];
      mx = fmax(mx, fabs(v));
    }
  }
  for (int b = threadIdx.x; b < (D.n_mp + 63) / 64; b += 256) mx = fmax(mx, D.pmax[b]);
  s_m[threadIdx.x] = mx;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) s_m[threadIdx.x] = fmax(s_m[threadIdx.x], s_m[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[w].lambda = 1e-5 * s_m[0];
}

}  // namespace vieo
