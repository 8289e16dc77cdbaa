// lba_solve_device.h -- the reduced-system solves of the bundle-adjustment engine (lba.hip), one per solver class
// (LbaDev::solver, the host's solver_class), each ending in lba_apply_step: x -> xp, the pose part of the gain-ratio
// scale, push() + oplus on the free key frames.  All under LBA_TRIAL.  The constants and size functions between the
// kernels (kLdP .. kLd16MaxFree, ld16_lds_bytes, kLdG*, ldg_lds_bytes, ldg_scratch_doubles, kNB, kBigLd) are the launch
// contract the host driver sizes its grids, LDS and scratch by.
//   k_lba_ldlt16     one workgroup per window: the reduced system formed in LDS (no Hs), its blocked LDL^T (FP64
//                    MFMA), solve, pose retraction (with backup) and the pose part of the gain-ratio scale.
//                    (windows) x kLd16Threads, LDS ld16_lds_bytes(blocks of the largest system) + 576 B; launch_round
//   k_lba_ldltg      the same left-looking, the factor in L2 as 16 x 16 blocks, for systems of 160 .. 639 unknowns.
//                    (windows) x kLdGThreads, LDS ldg_lds_bytes(..) + 48 B, factor in Hb (ldg_scratch_doubles); launch_round
//   k_big_*          the tiled LDL^T over many workgroups beyond that (full BA), dense or over the stored tiles of the
//                    symbolic fill pattern (gba_sparse_plan.h).  256 threads; k_big_init (nb^2 / 256, windows) from
//                    launch_round, panel / syrk / back_step / finish from launch_big_ldlt with the grids it is given
// Reads   Hs, bs (classes 1, 2), through lba_schur_device.h's entry functions Sp, Hpp, bp, sc_sys, Ae and the links (class
//         0), nb, nt, the plan's col_ptr / row_* / upd*, bfull, kf, n_kf, pd, scale_opt, out[w].lambda.
// Writes  Hb, Wp, big_fail, bfull (class 0), xp, kf, kf_bak, xf, scl, out[w].ok / scale_p.
#pragma once
#include "lba_schur_device.h"

namespace vieo {

// ---- dense LDL^T solve of the reduced system + pose update.
// The end of a solve, shared by the single-workgroup LDL^T and the tiled one: x -> D.xp, the pose part of
// computeScale(), push() + oplus on the free key frames.  y: the solution (LDS or global), 256 threads.
// NT: threads of the workgroup; the first 256 do the work (and sum in the same order whatever NT is).
template <int NT = 256>
__device__ __forceinline__ void lba_apply_step(const LbaDev& D, const double* y, double lambda, bool ok, WinOut& o,
                                               double* s_red, int tid) {
  const int n = D.np;
  double sp[1] = {0};
  if (tid < 256)
    for (int i = tid; i < n; i += 256) {
      D.xp[i] = y[i];
      sp[0] += y[i] * (lambda * y[i] + D.bfull[i]);  // pose part of computeScale()
    }
  if (NT == 256)
    block_sum<1>(sp, s_red, tid);
  else {
    sp[0] = wave_sum_d(sp[0]);
    __syncthreads();
    if ((tid & 63) == 0 && tid < 256) s_red[tid >> 6] = sp[0];
    __syncthreads();
    sp[0] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
  }
  if (tid == 0) {
    o.ok = ok ? 1 : 0, o.scale_p = ok ? sp[0] : 0.0;
    if (D.scale_opt) D.scl[1] = D.scl[0], D.scl[0] += y[n - 1];  // push(), VertexScale::oplusImpl (g2otypes.h:310)
  }
  if (tid >= 256) return;
  // oplus on the free key frames (push() first): VertexNavStatePR (+ V, Bias in a visual-inertial window)
  for (int k = tid; k < D.n_kf; k += 256) {
    LbaKf kf = D.kf[k];
    if (kf.col < 0) continue;
    D.kf_bak[k] = kf;
    Est e;
    e.p[0] = kf.p[0], e.p[1] = kf.p[1], e.p[2] = kf.p[2];
    e.qw = kf.qw, e.qx = kf.qx, e.qy = kf.qy, e.qz = kf.qz;
    inc_small_pr(e, y + kf.col);
    kf.p[0] = e.p[0], kf.p[1] = e.p[1], kf.p[2] = e.p[2];
    kf.qw = e.qw, kf.qx = e.qx, kf.qy = e.qy, kf.qz = e.qz;
    if (D.pd == 15)
      for (int a = 0; a < 3; a++)
        kf.v[a] += y[kf.col + 6 + a], kf.dbg[a] += y[kf.col + 9 + a], kf.dba[a] += y[kf.col + 12 + a];
    D.kf[k] = kf;
    write_kf_xf(D, k, kf);
  }
}

__device__ __forceinline__ double big_readlane(double v, int srclane) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)b, srclane);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), srclane);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// block t of a lower triangle counted row by row -> (row, column)
struct TriMap {
  unsigned char i[64], j[64];
  constexpr TriMap() : i(), j() {
    int t = 0;
    for (int r = 0; r < 11 && t < 64; r++)
      for (int c = 0; c <= r && t < 64; c++, t++) i[t] = (unsigned char)r, j[t] = (unsigned char)c;
  }
};
__constant__ TriMap kTriMap;

// ---- the same solve for reduced systems of up to 159 unknowns (ten key frames of a visual-inertial window, 26 of a
// vision-only one), blocked by 16 on the FP64 matrix cores.  The lower triangle of [H b; b^T 1] lives in LDS as
// 16 x 16 blocks (row pitch 17): row n carries the right-hand side, so the forward substitution falls out of the
// factorisation.  Per block column k, two phases with a barrier each:
//   panel      one thread per row below: W = A_ik L_kk^-T (un-normalised, kept in sWp), L_ik = W D_k^-1 in place
//   trailing   A_ij -= W_ik L_jk^T, one v_mfma_f64_16x16x4_f64 chain of four per block, blocks dealt over the
//              four wavefronts; wavefront 0 takes A_(k+1)(k+1) first and factorises it in registers right after
//              (one lane per row, v_readlane for the column broadcasts), hidden behind the other wavefronts' blocks
// then L^T x = z from the bottom block up (wavefront 0 solves the 16 x 16 triangle, the others fold the block into
// the earlier entries of z).
// Measured (MI355X, 150 unknowns, s_memtime inside the kernel): 75 us per solve against 200 us for the column-panel
// kernel above -- load 8.5, per block column 1.9 (panel) + 3.2 .. 5.2 (diagonal factor 2.7 on the critical path),
// back substitution 7.8, pose update 4.3 (the load then copied a ready Hs from HBM; forming the system there instead costs
// about 0.58 ms more of this kernel per 205-window step and saves 1.05 ms of k_lba_assemble).  What did NOT help: DPP row_newbcast instead of v_readlane in the
// diagonal factor (5.8 us instead of 2.9), letting every wavefront walk the whole block list and skip the blocks
// of the others (the scalar loop of 16 wavefronts serialises on the CU's scalar unit: +3.5 us at k = 0).
static const int kLdP = 17, kLdBlk = 16 * kLdP, kLd16MaxBlocks = 10, kLd16Threads = 1024;
static const int kLd16MaxFree = 27;  // free key frames of a system of up to 159 unknowns (6 per key frame at least)

__device__ __forceinline__ int ld16_blk(int i, int j) { return (i * (i + 1) / 2 + j) * kLdBlk; }

static size_t ld16_lds_bytes(int nbm) { return ((size_t)(nbm * (nbm + 1) / 2 + nbm) * kLdBlk + 16 + nbm * 16) * 8; }

template <int NT>
__global__ void __launch_bounds__(NT)
k_lba_ldlt16(const LbaDev* __restrict__ devs, const WinCtl* __restrict__ ctl, WinOut* __restrict__ out, int nb_max) {
  extern __shared__ __attribute__((aligned(16))) double s_dyn[];
  __shared__ double s_red[4];
  __shared__ int s_bad;
  __shared__ int s_link[5 * kLd16MaxFree];
  constexpr int NW = NT / 64;
  const int w = blockIdx.x;
  if (!(ctl[w].flags & LBA_TRIAL)) return;
  const LbaDev& D = devs[w];
  if (D.solver != 0) return;
  const int n = D.np, tid = threadIdx.x, lane = tid & 63;
  // wave-uniform for the compiler: the MFMA blocks of the other wavefronts must be branched over, not masked
  // (v_mfma ignores EXEC and would run its passes anyway)
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (n == 0) {
    if (tid == 0) out[w].ok = 1, out[w].scale_p = 0;
    return;
  }
  const double lambda = win_lambda(ctl[w], out[w]);
  const int nb = (n + 16) >> 4;  // blocks of the bordered matrix, n + 1 rows
  double* sA = s_dyn;
  double* sWp = sA + (size_t)(nb_max * (nb_max + 1) / 2) * kLdBlk;
  double* sD = sWp + (size_t)nb_max * kLdBlk;
  double* y = sD + 16;
  if (tid == 0) s_bad = 0;
  {  // The reduced system is formed HERE, from the Schur partials and the build's blocks, entry by entry through
    // lba_assemble_entry_at / lba_assemble_rhs_at (the functions k_lba_assemble runs for the other solver classes: the
    // same sums in the same order) -- no Hs in HBM, no launch.  Only the blocks on and below the diagonal.  The key
    // frames' pair-edge links are staged in LDS first, so that no entry waits for a chain of dependent loads; the
    // visual x visual entries, which carry the ns partials, are enumerated on their own (row fastest: the partials
    // of a wavefront's entries are contiguous), so that every thread takes its share of them.
    const int pd = D.pd, npv = D.npv, ksplit = D.ksplit;
    const int nchunks = (D.n_mp + kChunkLm - 1) / kChunkLm, cps = (nchunks + ksplit - 1) / ksplit;
    const int ns = (nchunks + cps - 1) / cps;  // k_lba_schur's split arithmetic
    if ((pd == 15 || D.n_imu > 0) && tid < D.n_free) lba_links_stage(D, tid, s_link);
    __syncthreads();
    const LbaLinksLds L{s_link};
    const float inv_v = 1.0f / (float)max(npv, 1), inv_n = 1.0f / (float)n, inv_pd = 1.0f / (float)pd;
    for (int e = tid; e < npv * npv; e += NT) {
      const int vc = (int)(((float)e + 0.5f) * inv_v), vr = e - vc * npv;  // exact: npv * npv < 2^15
      const int a = vr / 6, ra = vr - 6 * a, b = vc / 6, cb = vc - 6 * b;
      const int r = pd * a + ra, c = pd * b + cb;  // (the scale vertex: visual row 6 n_free = row pd n_free)
      if ((c >> 4) > (r >> 4)) continue;
      sA[ld16_blk(r >> 4, c >> 4) + (r & 15) * kLdP + (c & 15)] = lba_assemble_entry_at<false>(D, L, r, c, a, ra, b, cb, lambda, ns);
    }
    if (pd > 6)  // the entries with a velocity / bias row or column: pair edges and lambda only
      for (int i = tid; i < n * n; i += NT) {
        const int r = (int)(((float)i + 0.5f) * inv_n), c = i - r * n;  // exact: n * n < 2^15
        const int a = (int)(((float)r + 0.5f) * inv_pd), ra = r - a * pd, b = (int)(((float)c + 0.5f) * inv_pd), cb = c - b * pd;
        if ((c >> 4) > (r >> 4) || (ra < 6 && cb < 6)) continue;
        sA[ld16_blk(r >> 4, c >> 4) + (r & 15) * kLdP + (c & 15)] = lba_assemble_entry_at<false>(D, L, r, c, a, ra, b, cb, lambda, ns);
      }
    // border: row n = (b - S[:, npv])^T with pivot 1 (b itself -> bfull, for the gain ratio), identity padding below
    if (tid < n) {
      const int r = tid, a = (int)(((float)r + 0.5f) * inv_pd), ra = r - a * pd;
      double g, t;
      lba_assemble_rhs_at<false>(D, L, r, a, ra, ns, g, t);
      D.bfull[r] = g;
      sA[ld16_blk(n >> 4, r >> 4) + (n & 15) * kLdP + (r & 15)] = g - t;
    }
    const int rows = nb * 16 - n;
    for (int i = tid; i < rows * nb * 16; i += NT) {
      const int r = n + i / (nb * 16), c = i % (nb * 16);
      if ((c >> 4) > (r >> 4) || (r == n && c < n)) continue;
      const double v = r == c ? 1.0 : 0.0;
      sA[ld16_blk(r >> 4, c >> 4) + (r & 15) * kLdP + (c & 15)] = v;
    }
    // columns >= n of the rows above the border in the last block column
    for (int i = tid; i < 16 * 16; i += NT) {
      const int r = (n >> 4) * 16 + (i >> 4), c = (n >> 4) * 16 + (i & 15);
      if (r < n && c >= n) sA[ld16_blk(n >> 4, n >> 4) + (r & 15) * kLdP + (c & 15)] = 0.0;
    }
  }
  __syncthreads();
  typedef double double4_t __attribute__((ext_vector_type(4)));
  // A_kk = L D L^T in the registers of wavefront 0 (lanes 16..63 mirror lanes 0..15 so that the readlanes stay
  // wave-uniform); 1 / d_c (v_rcp_f64 + two Newton steps) goes to sD for the panel
  auto factor_diag = [&](int k) {
    double* Akk = sA + ld16_blk(k, k);
    const int r = lane & 15;
    double a[16];
#pragma unroll
    for (int c = 0; c < 16; c++) a[c] = Akk[r * kLdP + c];
    bool bad = false;
#pragma unroll
    for (int c = 0; c < 16; c++) {
      const double d = big_readlane(a[c], c);
      if (!(d > 0) && k * 16 + c < n) bad = true;  // the right-hand-side row and the padding are not pivots
      double inv = __builtin_amdgcn_rcp(d);
      inv = __builtin_fma(__builtin_fma(-d, inv, 1.0), inv, inv);
      inv = __builtin_fma(__builtin_fma(-d, inv, 1.0), inv, inv);
      const double l = a[c] * inv;
#pragma unroll
      for (int q = c + 1; q < 16; q++) a[q] -= l * big_readlane(a[c], q);  // w_q = A[q][c], un-normalised
      if (r > c) a[c] = l;
      if (r == c) a[c] = inv;
    }
    if (lane < 16) {
#pragma unroll
      for (int c = 0; c < 16; c++) {
        if (c < r) Akk[r * kLdP + c] = a[c];
        if (c == r) sD[c] = a[c];
      }
      if (bad) s_bad = 1;
    }
  };
  if (wv == 0) factor_diag(0);
  __syncthreads();
  bool ok = true;
  for (int k = 0; k < nb; k++) {
    if (s_bad) {
      ok = false;
      break;
    }
    const double* Akk = sA + ld16_blk(k, k);
    if (tid < (nb - k - 1) * 16) {
      const int i = k + 1 + (tid >> 4), r = tid & 15;
      double* src = sA + ld16_blk(i, k) + r * kLdP;
      double a[16];
#pragma unroll
      for (int c = 0; c < 16; c++) a[c] = src[c];
      // W L_kk^T = A: W[c] = A[c] - sum_{m < c} W[m] L_kk[c][m]   (LDS reads are broadcasts)
#pragma unroll
      for (int c = 1; c < 16; c++) {
        double v = a[c];
#pragma unroll
        for (int m = 0; m < c; m++) v -= a[m] * Akk[c * kLdP + m];
        a[c] = v;
      }
      double* wp = sWp + i * kLdBlk + r * kLdP;
#pragma unroll
      for (int c = 0; c < 16; c++) {
        wp[c] = a[c];
        src[c] = a[c] * sD[c];
      }
    }
    __syncthreads();
    // trailing update; the wavefront that owns A_(k+1)(k+1) factorises it straight away, one step ahead
    const int m = nb - k - 1;
    for (int t = wv; t < m * (m + 1) / 2; t += NW) {
      const int i = k + 1 + kTriMap.i[t], j = k + 1 + kTriMap.j[t];
      double* C = sA + ld16_blk(i, j) + (lane >> 4) * kLdP + (lane & 15);
      double4_t acc;
#pragma unroll
      for (int q = 0; q < 4; q++) acc[q] = C[q * 4 * kLdP];
      const double* pa = sWp + i * kLdBlk + (lane & 15) * kLdP + (lane >> 4);
      const double* pb = sA + ld16_blk(j, k) + (lane & 15) * kLdP + (lane >> 4);
#pragma unroll
      for (int ks = 0; ks < 4; ks++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-pa[ks * 4], pb[ks * 4], acc, 0, 0, 0);
#pragma unroll
      for (int q = 0; q < 4; q++) C[q * 4 * kLdP] = acc[q];
      if (t == 0) factor_diag(k + 1);  // wavefront 0; its own LDS traffic is in order
    }
    __syncthreads();
  }
  if (ok) {
    // z = D^-1 L^-1 b is row n of the factor; L^T x = z from the bottom block up.  Wavefront 0 folds x of block
    // kb + 1 into block kb and solves its triangle at once, the others fold it into the entries above.
    for (int i = tid; i < nb * 16; i += NT) y[i] = i < n ? sA[ld16_blk(n >> 4, i >> 4) + (n & 15) * kLdP + (i & 15)] : 0.0;
    __syncthreads();
    const int top = (n - 1) >> 4;
    for (int kb = top; kb >= 0; kb--) {
      if (wv == 0) {
        const int r = lane & 15, j = kb * 16 + r;
        double s = y[j];
        if (kb < top) {
          const double* blk = sA + ld16_blk(kb + 1, kb) + r;
#pragma unroll
          for (int q = 0; q < 16; q++) s -= blk[q * kLdP] * y[(kb + 1) * 16 + q];  // entries >= n are zero
        }
        const double* Akk = sA + ld16_blk(kb, kb);
        double Lc[16];
#pragma unroll
        for (int rr = 1; rr < 16; rr++) Lc[rr] = (r < rr && kb * 16 + rr < n) ? Akk[rr * kLdP + r] : 0.0;
#pragma unroll
        for (int rr = 15; rr >= 1; rr--) s -= Lc[rr] * big_readlane(s, rr);
        if (lane < 16 && j < n) y[j] = s;
      } else if (kb < top && tid - 64 < kb * 16) {
        const int j = tid - 64;
        const double* blk = sA + ld16_blk(kb + 1, j >> 4) + (j & 15);
        double v = y[j];
#pragma unroll
        for (int q = 0; q < 16; q++) v -= blk[q * kLdP] * y[(kb + 1) * 16 + q];
        y[j] = v;
      }
      __syncthreads();
    }
  } else {
    for (int i = tid; i < n; i += NT) y[i] = 0;
    __syncthreads();
  }
  lba_apply_step<NT>(D, y, lambda, ok, out[w], s_red, tid);
}

// ---- the same solve for reduced systems of 160 .. 639 unknowns (a bLarge window: 25 key frames x 15 = 375; a vision-only
// window of up to 106 key frames), one workgroup per window.  The lower triangle no longer fits LDS (567 KB at 375), so
// the factor lives in global memory -- L2-resident, 1.2 MB -- as 16 x 16 blocks stored COLUMN-major: lane l of a
// v_mfma_f64_16x16x4_f64 operand is element [l & 15][4 ks + (l >> 4)] of its block, i.e. double ks * 64 + l, so every
// operand load of a wavefront is one contiguous 512-byte read.  LEFT-looking by block column k:
//   gather     A_ik - sum_{j<k} W_ij L_kj^T for the row blocks i >= k: a chain of 4 k MFMAs per block with the
//              accumulator in registers (nothing is written back until the block is final; the right-looking form
//              would read and write every trailing block at every step).  What bounds it is the L2 round trip per
//              operand group, so a wavefront takes up to three row blocks at a time and shares the L_kj operands
//              between them; results go to LDS in row layout
//   diagonal   wavefront 0 gathers A_kk alone and factorises it in registers while the others still gather (row per
//              lane, v_readlane broadcasts)
//   panel      one thread per row below: W = A L_kk^-T (un-normalised) and L = W D_k^-1 -> global, column-major blocks
// Row n of the bordered matrix [H b; b^T 1] carries the right-hand side (forward substitution for free); L^T x = z from
// the bottom block up as in k_lba_ldlt16.  Same-workgroup visibility of the global writes: the wavefronts of a
// workgroup share the CU's vector L1 (write-through), so the barrier's workgroup-scope fence is enough.
// It replaces the multi-workgroup tiled solve for this size class (6 x k_big_panel + 5 x k_big_syrk + 6 x k_big_back_step
// per trial: 1.1 ms for the 51 bLarge windows of a bench step) and the column-panel kernel crawling in L2 (2.4 ms).
static const int kLdGMaxBlocks = 40, kLdGThreads = 512;
static size_t ldg_lds_bytes(int nbm) { return ((size_t)(nbm + 1) * kLdBlk + 16 + (size_t)nbm * 16) * 8; }
static size_t ldg_scratch_doubles(int nbm) { return (size_t)nbm * (nbm + 1) / 2 * 256 * 2; }

// element (row, col), col <= row's block, of the bordered matrix [H b; b^T 1] with identity padding
__device__ __forceinline__ double ldg_bordered(const LbaDev& D, int n, int row, int col) {
  if (row < n) return col < n ? D.Hs[(size_t)row * n + col] : 0.0;
  if (row == n) return col < n ? D.bs[col] : (col == n ? 1.0 : 0.0);
  return row == col ? 1.0 : 0.0;
}

// CNT row blocks i0, i0 + step, ... of block column k: A_ik - sum_{j<k} W_ij L_kj^T -> sP (row layout).  Four j per
// round trip to L2: the 16 operand loads of L_kj serve all CNT blocks, the CNT x 16 of W_ij go out with them, then
// 16 CNT MFMAs on 2 CNT independent accumulators.
template <int CNT>
__device__ __forceinline__ void ldg_gather(const LbaDev& D, int n, int k, int i0, int step, const double* Wg,
                                           const double* Lg, double* sP, int lane) {
  typedef double double4_t __attribute__((ext_vector_type(4)));
  double4_t acc[CNT][2];
  const double* pw[CNT];
#pragma unroll
  for (int c = 0; c < CNT; c++) {
    const int i = i0 + c * step;
#pragma unroll
    for (int q = 0; q < 4; q++) acc[c][0][q] = ldg_bordered(D, n, i * 16 + (lane >> 4) + 4 * q, k * 16 + (lane & 15));
    acc[c][1] = (double4_t){0, 0, 0, 0};
    pw[c] = Wg + (size_t)(i * (i + 1) / 2) * 256 + lane;
  }
  const double* pl = Lg + (size_t)(k * (k + 1) / 2) * 256 + lane;
  for (int j0 = 0; j0 < k; j0 += 4) {
    double b[16], a[CNT][16];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const bool in = j0 + u < k;
      const size_t o = (size_t)(in ? j0 + u : 0) * 256;
#pragma unroll
      for (int ks = 0; ks < 4; ks++) {
        b[u * 4 + ks] = in ? pl[o + ks * 64] : 0.0;
#pragma unroll
        for (int c = 0; c < CNT; c++) a[c][u * 4 + ks] = in ? pw[c][o + ks * 64] : 0.0;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
      for (int ks = 0; ks < 4; ks++)
#pragma unroll
        for (int c = 0; c < CNT; c++)
          acc[c][u & 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[c][u * 4 + ks], b[u * 4 + ks], acc[c][u & 1], 0, 0, 0);
  }
#pragma unroll
  for (int c = 0; c < CNT; c++) {
    double* C = sP + (size_t)(i0 + c * step) * kLdBlk + (lane >> 4) * kLdP + (lane & 15);
#pragma unroll
    for (int q = 0; q < 4; q++) C[q * 4 * kLdP] = acc[c][0][q] + acc[c][1][q];
  }
}

template <int NT>
__global__ void __launch_bounds__(NT)
k_lba_ldltg(const LbaDev* __restrict__ devs, const WinCtl* __restrict__ ctl, WinOut* __restrict__ out, int nb_max) {
  extern __shared__ __attribute__((aligned(16))) double s_dyn[];
  __shared__ double s_red[4];
  __shared__ int s_bad;
  constexpr int NW = NT / 64;
  const int w = blockIdx.x;
  if (!(ctl[w].flags & LBA_TRIAL)) return;
  const LbaDev& D = devs[w];
  if (D.solver != 1) return;
  const int n = D.np, tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: MFMA blocks are branched over, not masked
  if (n == 0) {
    if (tid == 0) out[w].ok = 1, out[w].scale_p = 0;
    return;
  }
  const double lambda = win_lambda(ctl[w], out[w]);
  const int nb = (n + 16) >> 4;  // blocks of the bordered matrix, n + 1 rows
  double* sP = s_dyn;                         // [nb] the block column after the gather, row layout, pitch kLdP
  double* sKK = sP + (size_t)nb_max * kLdBlk;  // L_kk (unit lower)
  double* sD = sKK + kLdBlk;                   // 1 / d of the block's pivots
  double* y = sD + 16;
  // (plain generic pointers on purpose: with address_space(1) loads the kernel measured 523 instead of 405 us)
  double* Wg = D.Hb;                                           // un-normalised W = L D, blocks (i, j), j <= i
  double* Lg = Wg + (size_t)D.nb * (D.nb + 1) / 2 * 256;      // L (D.nb: block capacity of the window)
  if (tid == 0) s_bad = 0;
  __syncthreads();
  bool ok = true;
  for (int k = 0; k < nb; k++) {
    // ---- gather: wavefront 0 takes the diagonal block alone and factorises it at once; the others share the row
    // blocks below, up to three at a time with the L_kj operands loaded once for all of them
    if (wv == 0) {
      ldg_gather<1>(D, n, k, k, 0, Wg, Lg, sP, lane);
      // ---- diagonal block: A_kk = L D L^T in the registers of wavefront 0 (lanes 16..63 mirror lanes 0..15 so
      // that the readlanes stay wave-uniform); its own LDS traffic is in order
      const double* Akk = sP + (size_t)k * kLdBlk;
      const int r = lane & 15;
      double a[16];
#pragma unroll
      for (int c = 0; c < 16; c++) a[c] = Akk[r * kLdP + c];
      bool bad = false;
#pragma unroll
      for (int c = 0; c < 16; c++) {
        const double d = big_readlane(a[c], c);
        if (!(d > 0) && k * 16 + c < n) bad = true;  // the right-hand-side row and the padding are not pivots
        double inv = __builtin_amdgcn_rcp(d);
        inv = __builtin_fma(__builtin_fma(-d, inv, 1.0), inv, inv);
        inv = __builtin_fma(__builtin_fma(-d, inv, 1.0), inv, inv);
        const double l = a[c] * inv;
#pragma unroll
        for (int q = c + 1; q < 16; q++) a[q] -= l * big_readlane(a[c], q);  // w_q = A[q][c], un-normalised
        if (r > c) a[c] = l;
        if (r == c) a[c] = inv;
      }
      if (lane < 16) {
        double* Lkk = Lg + (size_t)(k * (k + 1) / 2 + k) * 256;
#pragma unroll
        for (int c = 0; c < 16; c++) {
          if (c < r) sKK[r * kLdP + c] = a[c], Lkk[c * 16 + r] = a[c];
          if (c == r) sD[c] = a[c];
        }
        if (bad) s_bad = 1;
      }
    } else {
      for (int i0 = k + wv; i0 < nb; i0 += 3 * (NW - 1)) {
        const int cnt = (nb - i0 + NW - 2) / (NW - 1);  // row blocks i0, i0 + NW - 1, ... below nb
        if (cnt >= 3)
          ldg_gather<3>(D, n, k, i0, NW - 1, Wg, Lg, sP, lane);
        else if (cnt == 2)
          ldg_gather<2>(D, n, k, i0, NW - 1, Wg, Lg, sP, lane);
        else
          ldg_gather<1>(D, n, k, i0, NW - 1, Wg, Lg, sP, lane);
      }
    }
    __syncthreads();
    if (s_bad) {
      ok = false;
      break;
    }
    // ---- panel: one thread per row below the diagonal block
    for (int t = tid; t < (nb - k - 1) * 16; t += NT) {
      const int i = k + 1 + (t >> 4), r = t & 15;
      const double* src = sP + (size_t)i * kLdBlk + r * kLdP;
      double a[16];
#pragma unroll
      for (int c = 0; c < 16; c++) a[c] = src[c];
      // W L_kk^T = A: W[c] = A[c] - sum_{m < c} W[m] L_kk[c][m]   (LDS reads are broadcasts)
#pragma unroll
      for (int c = 1; c < 16; c++) {
        double v = a[c];
#pragma unroll
        for (int m = 0; m < c; m++) v -= a[m] * sKK[c * kLdP + m];
        a[c] = v;
      }
      double* wg = Wg + (size_t)(i * (i + 1) / 2 + k) * 256 + r;
      double* lg = Lg + (size_t)(i * (i + 1) / 2 + k) * 256 + r;
#pragma unroll
      for (int c = 0; c < 16; c++) {
        wg[c * 16] = a[c];
        lg[c * 16] = a[c] * sD[c];
      }
    }
    __threadfence_block();
    __syncthreads();
  }
  if (ok) {
    // z = D^-1 L^-1 b is row n of the factor; L^T x = z from the bottom block up
    const int bn = n >> 4, rn = n & 15;
    for (int i = tid; i < nb * 16; i += NT)
      y[i] = i < n ? Lg[(size_t)(bn * (bn + 1) / 2 + (i >> 4)) * 256 + (i & 15) * 16 + rn] : 0.0;
    __syncthreads();
    const int top = (n - 1) >> 4;
    for (int kb = top; kb >= 0; kb--) {
      if (wv == 0) {
        const int r = lane & 15, j = kb * 16 + r;
        double s = y[j];
        if (kb < top) {
          const double* blk = Lg + (size_t)((kb + 1) * (kb + 2) / 2 + kb) * 256 + r * 16;
#pragma unroll
          for (int q = 0; q < 16; q++) s -= blk[q] * y[(kb + 1) * 16 + q];  // entries >= n are zero
        }
        const double* Lkk = Lg + (size_t)(kb * (kb + 1) / 2 + kb) * 256 + r * 16;
        double Lc[16];
#pragma unroll
        for (int rr = 1; rr < 16; rr++) Lc[rr] = (r < rr && kb * 16 + rr < n) ? Lkk[rr] : 0.0;
#pragma unroll
        for (int rr = 15; rr >= 1; rr--) s -= Lc[rr] * big_readlane(s, rr);
        if (lane < 16 && j < n) y[j] = s;
      } else if (kb < top) {
        for (int j = tid - 64; j < kb * 16; j += NT - 64) {
          const double* blk = Lg + (size_t)((kb + 1) * (kb + 2) / 2 + (j >> 4)) * 256 + (j & 15) * 16;
          double v = y[j];
#pragma unroll
          for (int q = 0; q < 16; q++) v -= blk[q] * y[(kb + 1) * 16 + q];
          y[j] = v;
        }
      }
      __syncthreads();
    }
  } else {
    for (int i = tid; i < n; i += NT) y[i] = 0;
    __syncthreads();
  }
  lba_apply_step<NT>(D, y, lambda, ok, out[w], s_red, tid);
}

// ---- tiled LDL^T for reduced systems that do not fit one workgroup (global BA: hundreds of key frames).
// Right-looking over 64-column panels of the padded lower triangle Hb [nb][nb]; row np carries the right-hand
// side, so the forward substitution falls out of the factorisation (its row of L is D^-1 L^-1 b).
//   k_big_init   Hb <- Hs, bs; identity on the padding
//   k_big_panel  step k: every workgroup factorises the 64 x 64 diagonal tile in LDS (redundantly: 87 kflop) and
//                solves its own 256 rows below it, one row per lane held in registers: W = A L_kk^-T -> Wp
//                (un-normalised), L = W D^-1 in place
//   k_big_syrk   A_ij -= W_ik L_jk^T for the tiles right of the panel: FP64 MFMA, 64 x 64 x 64 per workgroup
//   k_big_back_step  L^T x = z, one 64-row block per launch from the bottom; k_big_finish: lba_apply_step
// TILES = true (solver 3, the full BA's tile-sparse solve): the same kernels over the stored tiles of gba_sparse_plan.h
// (64 x 64 slots of the pool D.Hb, leading dimension 64; k_lba_assemble_tiles takes k_big_init's place): the panel's
// rows are those of the stored tiles below the diagonal one, the trailing update runs over the plan's targets of the
// panel, back-substitution skips the tiles that are not stored (they hold exact zeros in the dense matrix).
static const int kNB = 64, kBigLd = kNB + 2;

__global__ void __launch_bounds__(256)
k_big_init(const LbaDev* __restrict__ devs, const WinCtl* __restrict__ ctl) {
  const int w = blockIdx.y;
  if (!(ctl[w].flags & LBA_TRIAL)) return;
  const LbaDev& D = devs[w];
  if (D.solver != 2) return;
  const int n = D.np, nb = D.nb;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e == 0) *D.big_fail = 0;
  if (n == 0 || e >= (size_t)nb * nb) return;
  const int r = (int)(e / nb), c = (int)(e - (size_t)r * nb);
  if (c > r) return;
  double v = r == c ? (r == n ? 1e300 : 1.0) : 0.0;  // the right-hand-side row never limits a pivot
  if (r < n)
    v = D.Hs[(size_t)r * n + c];
  else if (r == n && c < n)
    v = D.bs[c];
  D.Hb[e] = v;
}

template <bool TILES>
__global__ void __launch_bounds__(256)
k_big_panel(const LbaDev* __restrict__ devs, const WinCtl* __restrict__ ctl, int k) {
  __shared__ double sA[kNB * kBigLd];  // the diagonal tile, then its unit-lower factor
  __shared__ double sD[kNB];
  const int w = blockIdx.y;
  if (!(ctl[w].flags & LBA_TRIAL)) return;
  const LbaDev& D = devs[w];
  if (D.solver != (TILES ? 3 : 2)) return;
  const int n = D.np, nb = D.nb, tid = threadIdx.x;
  const int r0 = (k + 1) * kNB + blockIdx.x * 256 - 256;  // block 0: the diagonal tile itself, then 256 rows each
  const int below = TILES && k < D.nt ? D.col_ptr[k + 1] - D.col_ptr[k] - 1 : 0;  // TILES: stored tiles under the diagonal one
  if (n == 0 || k * kNB >= nb || (blockIdx.x > 0 && (TILES ? (int)(blockIdx.x - 1) * 256 >= below * kNB : r0 >= nb))) return;
  double* Hb = D.Hb;
  const size_t ld = TILES ? kNB : nb;
  double* const dg = TILES ? Hb + (size_t)D.col_ptr[k] * kGbaTileElems : Hb + (size_t)(k * kNB) * ld + k * kNB;
  {  // the 16 loads of a thread in flight, then the LDS stores
    double v[16];
#pragma unroll
    for (int u = 0; u < 16; u++) {
      const int i = tid + 256 * u, r = i >> 6, c = i & 63;
      v[u] = c <= r ? dg[(size_t)r * ld + c] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 16; u++) {
      const int i = tid + 256 * u;
      sA[(i >> 6) * kBigLd + (i & 63)] = v[u];
    }
  }
  __syncthreads();
  // LDL^T of the tile by ONE wavefront, register resident: lane r holds row r, column c is broadcast with
  // v_readlane (no LDS traffic, no barriers); lanes r <= c carry don't-care values in a[q], q > r.
  bool bad = false;
  if (tid < kNB) {
    double a[kNB];
#pragma unroll
    for (int c = 0; c < kNB; c++) a[c] = sA[tid * kBigLd + c];
#pragma unroll
    for (int c = 0; c < kNB; c++) {
      const double d = big_readlane(a[c], c);
      if (!(d > 0) && k * kNB + c < n) bad = true;  // the right-hand-side row and the padding are not pivots
      const double l = a[c] / d;
#pragma unroll
      for (int q = c + 1; q < kNB; q++) a[q] -= l * big_readlane(a[c], q);  // w_q = A[q][c], un-normalised
      if (tid > c) a[c] = l;
    }
#pragma unroll
    for (int c = 0; c < kNB; c++) {
      if (c < tid) sA[tid * kBigLd + c] = a[c];
      if (c == tid) sD[c] = a[c];
    }
    if (bad && blockIdx.x == 0) *D.big_fail = 1;
  }
  __syncthreads();
  if (blockIdx.x == 0) {
    for (int i = tid; i < kNB * kNB; i += 256) {
      const int r = i >> 6, c = i & 63;
      if (c < r) dg[(size_t)r * ld + c] = sA[r * kBigLd + c];
      if (c == r) dg[(size_t)r * ld + c] = sD[c];
    }
    return;
  }
  int row;
  double* src;
  if (TILES) {
    const int q = (blockIdx.x - 1) * 256 + tid, p = D.col_ptr[k] + 1 + (q >> 6);
    if (q >= below * kNB) return;
    row = D.tile_i[p] * kNB + (q & 63);
    src = Hb + (size_t)p * kGbaTileElems + (q & 63) * kNB;
  } else {
    row = r0 + tid;
    if (row >= nb) return;
    src = Hb + (size_t)row * ld + k * kNB;
  }
  double a[kNB];
#pragma unroll
  for (int c = 0; c < kNB; c++) a[c] = src[c];
  // W L_kk^T = A: W[c] = A[c] - sum_{m < c} W[m] L_kk[c][m]   (LDS reads are broadcasts)
#pragma unroll
  for (int c = 1; c < kNB; c++) {
    double v = a[c];
#pragma unroll
    for (int m = 0; m < c; m++) v -= a[m] * sA[c * kBigLd + m];
    a[c] = v;
  }
  double* wp = D.Wp + (size_t)row * kNB;
#pragma unroll
  for (int c = 0; c < kNB; c++) {
    wp[c] = a[c];
    src[c] = a[c] / sD[c];
  }
}

template <bool TILES>
__global__ void __launch_bounds__(256)
k_big_syrk(const LbaDev* __restrict__ devs, const WinCtl* __restrict__ ctl, int k) {
  __shared__ __attribute__((aligned(16))) double sW[kNB * kBigLd];
  __shared__ __attribute__((aligned(16))) double sL[kNB * kBigLd];
  const int w = blockIdx.y;
  if (!(ctl[w].flags & LBA_TRIAL)) return;
  const LbaDev& D = devs[w];
  if (D.solver != (TILES ? 3 : 2)) return;
  const int nb = D.nb;
  if (D.np == 0) return;
  int bi, bj;
  size_t ld;
  double *Lt, *Tt;  // tile (bj, k) of L, the target tile (bi, bj)
  if (TILES) {  // the plan's targets of panel k
    if (k >= D.nt) return;
    const int u = D.upd_ptr[k] + blockIdx.x;
    if (u >= D.upd_ptr[k + 1]) return;
    const int* U = D.upd + 5 * (size_t)u;
    bi = U[0], bj = U[1], ld = kNB;
    Lt = D.Hb + (size_t)U[3] * kGbaTileElems, Tt = D.Hb + (size_t)U[4] * kGbaTileElems;
  } else {
    const int nt = nb / kNB, m = nt - k - 1;
    if (m <= 0) return;
    int t = blockIdx.x, ti = 0;  // tile (k + 1 + ti, k + 1 + tj), tj <= ti, row-major over the lower triangle
    if (t >= m * (m + 1) / 2) return;
    while (t > ti) t -= ti + 1, ti++;
    bi = k + 1 + ti, bj = k + 1 + t, ld = nb;
    Lt = D.Hb + (size_t)(bj * kNB) * ld + k * kNB, Tt = D.Hb + (size_t)(bi * kNB) * ld + bj * kNB;
  }
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  {  // both tiles in flight (32 loads per thread), then the LDS stores
    double vw[16], vl[16];
#pragma unroll
    for (int u = 0; u < 16; u++) {
      const int i = tid + 256 * u, r = i >> 6, c = i & 63;
      vw[u] = D.Wp[(size_t)(bi * kNB + r) * kNB + c];
      vl[u] = Lt[(size_t)r * ld + c];
    }
#pragma unroll
    for (int u = 0; u < 16; u++) {
      const int i = tid + 256 * u, r = i >> 6, c = i & 63;
      sW[r * kBigLd + c] = vw[u];
      sL[r * kBigLd + c] = vl[u];
    }
  }
  __syncthreads();
  typedef double double4_t __attribute__((ext_vector_type(4)));
  double4_t acc[4];
#pragma unroll
  for (int q = 0; q < 4; q++) acc[q] = (double4_t){0, 0, 0, 0};
  const double* pa = sW + (wv * 16 + (lane & 15)) * kBigLd + (lane >> 4);
  const double* pb = sL + (lane & 15) * kBigLd + (lane >> 4);
#pragma unroll
  for (int ks = 0; ks < kNB / 4; ks++) {
    const double av = pa[ks * 4];
#pragma unroll
    for (int q = 0; q < 4; q++)
      acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, pb[q * 16 * kBigLd + ks * 4], acc[q], 0, 0, 0);
  }
  // f64 C/D map: col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
  for (int q = 0; q < 4; q++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int lr = wv * 16 + (lane >> 4) + 4 * r, lc = q * 16 + (lane & 15);
      if (bj * kNB + lc <= bi * kNB + lr) Tt[(size_t)lr * ld + lc] -= acc[q][r];
    }
}

// step s of L^T x = z from the bottom: block kb = last - s.  Every workgroup solves the 64 x 64 block in LDS
// (one wavefront, redundantly); workgroup 0 publishes x of the block, the others fold it into their 256 columns
// of z (kept in Wp, free after the factorisation): z[c] -= sum_r L[c0 + r][c] x[r].
// TILES: the right-hand-side row lies in the last tile row, which is full; a column tile of row block kb that is not
// stored leaves its z untouched (the dense step subtracts exact zeros there).
template <bool TILES>
__global__ void __launch_bounds__(256)
k_big_back_step(const LbaDev* __restrict__ devs, const WinCtl* __restrict__ ctl, int s) {
  __shared__ double sA[kNB * kBigLd];
  __shared__ double sx[kNB];
  const int w = blockIdx.y;
  if (!(ctl[w].flags & LBA_TRIAL)) return;
  const LbaDev& D = devs[w];
  if (D.solver != (TILES ? 3 : 2)) return;
  const int n = D.np, nb = D.nb, tid = threadIdx.x;
  if (n == 0) return;
  const int kb = (n - 1) / kNB - s;
  if (kb < 0) return;
  const int c0 = kb * kNB, cn = min(kNB, n - c0);
  if (blockIdx.x > 0 && (int)(blockIdx.x - 1) * 256 >= c0) return;
  const size_t ld = TILES ? kNB : nb;
  // z = D^-1 L^-1 b: the right-hand-side row of L (step 0; TILES: the last stored tile of every column), then the
  // running values in Wp
  auto z = [&](int c) -> double {
    if (s != 0) return D.Wp[c];
    if (TILES) return D.Hb[(size_t)(D.col_ptr[(c >> 6) + 1] - 1) * kGbaTileElems + (n & 63) * kNB + (c & 63)];
    return D.Hb[(size_t)n * ld + c];
  };
  const double* dg = TILES ? D.Hb + (size_t)D.col_ptr[kb] * kGbaTileElems : D.Hb + (size_t)c0 * ld + c0;
  {
    double v[16];
#pragma unroll
    for (int u = 0; u < 16; u++) {
      const int i = tid + 256 * u, r = i >> 6, c = i & 63;
      v[u] = (c < r && r < cn) ? dg[(size_t)r * ld + c] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 16; u++) {
      const int i = tid + 256 * u;
      sA[(i >> 6) * kBigLd + (i & 63)] = v[u];
    }
  }
  if (tid < kNB) sx[tid] = tid < cn ? z(c0 + tid) : 0.0;
  __syncthreads();
  if (tid < kNB)  // x[r] is final once the rows below it have been applied
    for (int r = cn - 1; r > 0; r--) {
      const double xr = sx[r];
      if (tid < r) sx[tid] -= sA[r * kBigLd + tid] * xr;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  __syncthreads();
  if (blockIdx.x == 0) {
    if (tid < cn) D.xp[c0 + tid] = sx[tid];
    return;
  }
  const int c = (blockIdx.x - 1) * 256 + tid;
  if (c >= c0) return;
  double v = z(c);
  const double* Lc;  // column c of row block kb
  if (TILES) {
    const int J = c >> 6, end = D.row_ptr[kb + 1] - 1;  // (the last entry of the row is the diagonal tile)
    int lo = D.row_ptr[kb], hi = end;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (D.row_j[mid] < J)
        lo = mid + 1;
      else
        hi = mid;
    }
    if (lo == end || D.row_j[lo] != J) {
      D.Wp[c] = v;
      return;
    }
    Lc = D.Hb + (size_t)D.row_tile[lo] * kGbaTileElems + (c & 63);
  } else
    Lc = D.Hb + (size_t)c0 * ld + c;
  for (int r0 = 0; r0 < cn; r0 += 16) {  // 16 rows in flight; the subtraction order stays r ascending
    double l[16];
#pragma unroll
    for (int u = 0; u < 16; u++) l[u] = r0 + u < cn ? Lc[(size_t)(r0 + u) * ld] : 0.0;
#pragma unroll
    for (int u = 0; u < 16; u++)
      if (r0 + u < cn) v -= l[u] * sx[r0 + u];
  }
  D.Wp[c] = v;
}

template <bool TILES>
__global__ void __launch_bounds__(256)
k_big_finish(const LbaDev* __restrict__ devs, const WinCtl* __restrict__ ctl, WinOut* __restrict__ out) {
  __shared__ double s_red[4];
  const int w = blockIdx.x;
  if (!(ctl[w].flags & LBA_TRIAL)) return;
  const LbaDev& D = devs[w];
  if (D.solver != (TILES ? 3 : 2)) return;
  const int n = D.np, tid = threadIdx.x;
  if (n == 0) {
    if (tid == 0) out[w].ok = 1, out[w].scale_p = 0;
    return;
  }
  const bool ok = *D.big_fail == 0;
  if (!ok) {
    for (int i = tid; i < n; i += 256) D.xp[i] = 0;
    __syncthreads();
  }
  lba_apply_step(D, D.xp, win_lambda(ctl[w], out[w]), ok, out[w], s_red, tid);
}

}  // namespace vieo
