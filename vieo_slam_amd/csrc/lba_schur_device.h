// lba_schur_device.h -- the Schur product of the bundle-adjustment engine (lba.hip) and the reduced system's entries
// (g2o BlockSolver<6,3>, block_solver.hpp:353-589).  Grids are (x, windows) x 256 threads; launched by launch_round
// (lba.hip) under LBA_TRIAL (k_lba_occ: LBA_BEGIN).  kChunkLm is also the host's split arithmetic (schur_ksplit).
//   k_lba_occ        full BA only: which 16-landmark chunks a 64-row tile of BB touches; one thread per (tile, chunk)
//   k_lba_schur<OFFDIAG, TILES>  the Schur complement as what it is, a GEMM: (BB D^-1) x [BB; b_l]^T with
//                    D = blockdiag(H_ll + lambda I), K = 3 x points split over workgroups, 64x64 output
//                    tiles on the FP64 matrix cores (v_mfma_f64_16x16x4_f64); the dense operand tiles exist
//                    only in LDS: a K-chunk is staged from the compact blocks through `tab` (zeros where a key
//                    frame does not see a point), D^-1 applied on the way; per-split partial products.
//                    x = tiles x ksplit (diagonal / off-diagonal tiles, dense or the plan's), LDS 53504 B
//   k_lba_pack       landmark-sharded windows: this rank's Schur sums, H_pp, b_p, the scale's blocks -> red
//   k_lba_assemble   Hs = H_pp + lambda I - sum of the partials (fixed order), bs likewise: for the systems of 160
//                    unknowns and more (k_lba_ldltg, k_big_*); k_lba_ldlt16 forms its own through the same functions
//                    (lba_assemble_entry_at / lba_assemble_rhs_at).  Grid (entries / 256, windows of the solver class)
//   k_lba_assemble_tiles  the same entries into the tile pool Hb of the tile-sparse solve, bordered; clears big_fail
// Reads   tab, CB, Bs, bl, Hll, mp_act, occ, use_occ, ksplit, ldS, sp_stride, solver, the plan's sch_* / tile_i / tile_j,
//         Hpp, bp, sc_sys, Ae, imu, kf_list, kf_in, kf_out, red (after the all-reduce), out[w].lambda.
// Writes  occ, Sp, red, Hs, bs, bfull, Hb, big_fail.
#pragma once
#include "gba_sparse_plan.h"
#include "lba_device.h"

namespace vieo {

// ---- Schur complement GEMM.  S = (BB D^-1) [BB; bl]^T, S is np x (np + 1), tiled 64 x 64 (upper
// block-tiles only), K = 3 x points cut into chunks of 16 points; grid x = block-tile * ksplit + split.
typedef double double4_t __attribute__((ext_vector_type(4)));
static const int kChunkLm = 16, kLd = 3 * kChunkLm + 2;  // +2: conflict-free b64 fragment reads

// Which 16-landmark chunks a 64-row tile of BB touches (from `tab`, rebuilt at every optimize()): the Schur
// GEMM skips the all-zero ones -- a map of hundreds of key frames is block-sparse, a local window is dense.
__global__ void __launch_bounds__(256)
k_lba_occ(const LbaDev* __restrict__ devs, const WinCtl* __restrict__ ctl) {
  const int w = blockIdx.y;
  if (!(ctl[w].flags & LBA_BEGIN)) return;
  const LbaDev& D = devs[w];
  if (!D.use_occ) return;
  const int np = D.npv, CB = (np + 64) >> 6, nchunks = (D.n_mp + kChunkLm - 1) / kChunkLm;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (np == 0 || e >= CB * nchunks) return;
  const int bi = e / nchunks, ch = e - bi * nchunks;
  const int a0 = bi * 64 / 6, a1 = min((bi * 64 + 63) / 6, D.n_free - 1);
  int any = D.scale_opt && (np - 1) >= bi * 64 && (np - 1) < bi * 64 + 64;  // the scale's row sees every point
  for (int a = a0; a <= a1 && !any; a++)
    for (int j = 0; j < kChunkLm; j++) {
      const int m = ch * kChunkLm + j;
      if (m < D.n_mp && D.tab[(size_t)a * D.n_mp + m] >= 0) {
        any = 1;
        break;
      }
    }
  D.occ[e] = (unsigned char)any;
}

// Two instances: the diagonal tiles (bi == bj: one register set of blocks, three wavefronts per SIMD = the three
// workgroups a CU's LDS holds) and the off-diagonal ones (two register sets; at 168 registers they spilled the blocks
// they had just loaded, i.e. waited for them at once: two wavefronts per SIMD).  An ordinary window is one diagonal tile.
// TILES (tile-sparse solve, solver 3): the tiles of the plan's lists instead of the whole upper triangle, each one's
// partial product into its own 64 x 64 slot of Sp; the body is the same.
template <bool OFFDIAG, bool TILES = false>
__global__ void __launch_bounds__(256, OFFDIAG ? 2 : 3)
k_lba_schur(const LbaDev* __restrict__ devs, const WinCtl* __restrict__ ctl, const WinOut* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) double sT[64 * kLd];
  __shared__ __attribute__((aligned(16))) double sB[64 * kLd];
  __shared__ double sDi[2][kChunkLm * 9];
  const int w = blockIdx.y;
  if (!(ctl[w].flags & LBA_TRIAL)) return;
  const LbaDev& D = devs[w];
  const int np = D.npv;  // the landmarks touch the PR blocks only
  if (np == 0) return;
  const int RB = (np + 63) >> 6, CB = (np + 64) >> 6;  // CB covers the extra column bl
  const int ksplit = D.ksplit;
  int bt = blockIdx.x / ksplit;
  const int split = blockIdx.x % ksplit;
  int bi = 0, bj;
  if (TILES != (D.solver == 3)) return;
  if (TILES) {
    if (bt >= (OFFDIAG ? D.n_sch_off : D.n_sch_diag)) return;
    bt = (OFFDIAG ? D.sch_off : D.sch_diag)[bt];  // the tile's slot
    bi = D.sch_i[bt], bj = D.sch_j[bt];
  } else if (OFFDIAG) {  // tiles (bi, bj), bi < bj < CB, row by row
    while (bi < RB && bt >= CB - bi - 1) bt -= CB - bi - 1, bi++;
    if (bi >= RB) return;
    bj = bi + 1 + bt;
  } else {
    if (bt >= RB) return;
    bi = bj = bt;
  }
  const int nchunks = (D.n_mp + kChunkLm - 1) / kChunkLm, cps = (nchunks + ksplit - 1) / ksplit;
  const int c0 = split * cps, c1 = min(nchunks, c0 + cps);
  if (c0 >= c1) return;  // k_lba_assemble uses the same split arithmetic
  const double lambda = win_lambda(ctl[w], out[w]);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n_mp = D.n_mp;
  double4_t acc[4];
#pragma unroll
  for (int q = 0; q < 4; q++) acc[q] = (double4_t){0, 0, 0, 0};
  // Diagonal tiles: the 16 x 16 blocks (i, j) that somebody reads, dealt over the wavefronts.  Every reader of Sp
  // (lba_schur_sum, k_lba_pack) takes entry (min(r, c), max(r, c)) with r < npv, or (r, npv), so block (i, j) of tile
  // (bi, bi) is needed iff i <= j, its rows start below the last valid row (16 i < npv - 64 bi) and its columns start
  // at or before column npv, which carries b_l (16 j <= npv - 64 bi): 10 of a full tile's 16.  EVERY OTHER BLOCK OF
  // A DIAGONAL TILE OF Sp IS UNDEFINED (never written).  The needed blocks, counted row by row, go round the
  // wavefronts -- {00 11 23} {01 12 33} {02 13} {03 22} for a full tile, at most three each (dealing the odd splits from
  // wavefront 3 down, to load a CU's four SIMDs alike, measured 1 % slower).  Which wavefront issues a block's MFMAs
  // does not change them: chunks ascending, ks ascending, the same LDS words.
  // Off-diagonal tiles: every row is valid (bi < bj), and only the column rule bites -- in the last column tile the
  // blocks beyond column npv's are neither computed nor stored (nq of the four; workgroup-uniform).
  const int nq = min(4, ((np - 64 * bj) >> 4) + 1);
  int nblk = 0, bi0 = 0, bj0 = 0, bi1 = 0, bj1 = 0, bi2 = 0, bj2 = 0;  // this wavefront's blocks (wave-uniform)
  if (!OFFDIAG) {
    const int left = np - 64 * bi;
    int k = 0;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = i; j < 4; j++)
        if (16 * i < left && 16 * j <= left) {
          if ((k & 3) == wv) {
            if (nblk == 0) bi0 = i, bj0 = j;
            if (nblk == 1) bi1 = i, bj1 = j;
            if (nblk == 2) bi2 = i, bj2 = j;
            nblk++;
          }
          k++;
        }
  }
  const unsigned char* occ_i = D.occ + (size_t)bi * nchunks;
  const unsigned char* occ_j = D.occ + (size_t)bj * nchunks;
  const bool has_bl = np >= bj * 64 && np < bj * 64 + 64;  // this column tile carries b_l: dense
  // the chunks this workgroup works on: a zero factor adds nothing (workgroup-uniform)
  // (local windows: every chunk -- the flag bytes would be one more dependent global load per chunk)
  const bool use_occ = D.use_occ != 0;
  auto next_chunk = [&](int ch) {
    if (use_occ)
      while (ch < c1 && (!occ_i[ch] || (!has_bl && !occ_j[ch]))) ch++;
    return ch;
  };
  // Staging.  The operand tiles T = (BB D^-1)[rows of tile bi] and B = [BB; b_l][rows of tile bj], 64 x 48 per chunk
  // of 16 landmarks, exist only in LDS.  One thread per (key-frame slot of the tile, landmark of the chunk) pair --
  // 12 slots cover the 64 rows whatever 6 a mod 64 is: wavefronts 0..2 -- looks the pair's edge up in `tab` and writes
  // its 6 x 3 block or zeros: nothing to clear, two barriers per chunk.  The slot after the last free key frame carries
  // the scale vertex's row (bScaleOpt) and, on the B side, the extra column b_l.  Wavefront 3 has no pairs: its first
  // 16 lanes form (H_ll + lambda I)^-1 of the NEXT chunk's landmarks while the others stage the current one.
  // Software pipeline: blocks of chunk c + 1 in registers, `tab` entries of chunk c + 2, H_ll of chunk c + 2.
  // The loop has NO load whose address or predicate depends on another load of the same iteration (s_memtime probes,
  // tools/probe_schur.sh: such a chain -- activity byte -> H_ll, tab entry -> "edge present?" branch -> block -- put a
  // full vmcnt(0) wait, i.e. the whole HBM latency, into every chunk: 16.5 k cycles per chunk against 2.9 k of MFMAs).
  // Absent pairs read a zero block (CB[n_obs], cleared by k_lba_zero) instead of branching, indices are clamped
  // instead of guarded, predicates are applied to the VALUES.
  typedef double dbl2_t __attribute__((ext_vector_type(2)));
  typedef const dbl2_t __attribute__((address_space(1)))* gd2p;
  typedef const double __attribute__((address_space(1)))* gdp;
  typedef const int __attribute__((address_space(1)))* gip;
  typedef const unsigned char __attribute__((address_space(1)))* gbp;
  const gd2p gCB = (gd2p)D.CB;
  const gdp gBs = (gdp)D.Bs, gbl = (gdp)D.bl, gHll = (gdp)D.Hll;
  const gip gtab = (gip)D.tab;
  const gbp gact = (gbp)D.mp_act;
  const int ps = tid >> 4, pj = tid & 15;
  const int nfree = D.n_free, n_obs = D.n_obs;
  const bool sc_opt = D.scale_opt != 0;
  constexpr bool offdiag = OFFDIAG;
  const int aT = (64 * bi) / 6 + ps, aB = (64 * bj) / 6 + ps;
  const int rT = 6 * aT - 64 * bi, rB = 6 * aB - 64 * bj;  // tile row of the pair's first row (-5 .. 66)
  const int aTc = min(aT, max(nfree, 1) - 1), aBc = min(aB, max(nfree, 1) - 1);
  // does this wavefront hold the slot after the last key frame (per side)?  wave-uniform
  const bool spT = wv < 3 && nfree >= (64 * bi) / 6 + 4 * wv && nfree < (64 * bi) / 6 + 4 * wv + 4;
  const bool spB = wv < 3 && nfree >= (64 * bj) / 6 + 4 * wv && nfree < (64 * bj) / 6 + 4 * wv + 4;
  auto tab_of = [&](int a, int ac, int ch) -> int {  // unconditional load, the predicate picks the value
    const int m = ch * kChunkLm + pj;
    const int t = gtab[(size_t)ac * n_mp + min(m, n_mp - 1)];
    return (ch < c1 && a < nfree && m < n_mp) ? t : -1;
  };
  auto load_blk = [&](int e, double* v) {  // e < 0: the zero block
    const gd2p p = gCB + 9 * (size_t)min((unsigned)e, (unsigned)n_obs);
#pragma unroll
    for (int t = 0; t < 9; t++) {
      const dbl2_t x = p[t];
      v[2 * t] = x[0], v[2 * t + 1] = x[1];
    }
  };
  // the slot after the last key frame: the scale vertex's row and b_l of the landmark (zeros for the other threads)
  auto load_special = [&](int a, int ch, bool with_bl, double* sp, double* blv) {
    const int m = ch * kChunkLm + pj, mc = min(m, n_mp - 1);
    const bool mine = a == nfree && m < n_mp && ch < c1;
    double s0 = 0, s1 = 0, s2 = 0;
    if (sc_opt) s0 = gBs[3 * (size_t)mc], s1 = gBs[3 * (size_t)mc + 1], s2 = gBs[3 * (size_t)mc + 2];
    sp[0] = mine ? s0 : 0.0, sp[1] = mine ? s1 : 0.0, sp[2] = mine ? s2 : 0.0;
    if (with_bl) {
      const double b0 = gbl[3 * (size_t)mc], b1 = gbl[3 * (size_t)mc + 1], b2 = gbl[3 * (size_t)mc + 2];
      const bool on = mine && gact[mc] != 0;
      blv[0] = on ? b0 : 0.0, blv[1] = on ? b1 : 0.0, blv[2] = on ? b2 : 0.0;
    }
  };
  double ta[18], tb[18], spT3[3] = {0, 0, 0}, spB3[3] = {0, 0, 0}, blv[3] = {0, 0, 0}, hl[9];
  unsigned char hl_on = 0;
  auto load_hll = [&](int ch) {  // wavefront 3, lanes 0..15 (the others load the same clamped landmark)
    const int m = ch * kChunkLm + (lane & 15), mc = min(m, n_mp - 1);
#pragma unroll
    for (int t = 0; t < 9; t++) hl[t] = gHll[9 * (size_t)mc + t];
    hl_on = (ch < c1 && m < n_mp) ? gact[mc] : (unsigned char)0;
  };
  auto store_dinv = [&](int buf) {  // wavefront 3, lanes 0..15
    double Di[9];
    landmark_dinv(hl, lambda, Di);
    if (lane < kChunkLm) {
#pragma unroll
      for (int t = 0; t < 9; t++) sDi[buf][lane * 9 + t] = hl_on ? Di[t] : 0.0;
    }
  };
  // rows of the pair -> LDS (a slot that straddles the tile's edge has rows outside it)
  auto stage_T = [&](const double* v, const double* Di) {
    const double d0 = Di[0], d1 = Di[1], d2 = Di[2], d3 = Di[3], d4 = Di[4], d5 = Di[5], d6 = Di[6], d7 = Di[7], d8 = Di[8];
#pragma unroll
    for (int q = 0; q < 6; q++) {
      const unsigned r = (unsigned)(rT + q);
      if (r < 64u) {
        double b0 = v[3 * q], b1 = v[3 * q + 1], b2 = v[3 * q + 2];
        if (q == 0) b0 += spT3[0], b1 += spT3[1], b2 += spT3[2];  // the scale vertex's row (zeros elsewhere)
        double* d = sT + r * kLd + 3 * pj;
        d[0] = __builtin_fma(b2, d6, __builtin_fma(b1, d3, b0 * d0));
        d[1] = __builtin_fma(b2, d7, __builtin_fma(b1, d4, b0 * d1));
        d[2] = __builtin_fma(b2, d8, __builtin_fma(b1, d5, b0 * d2));
      }
    }
  };
  auto stage_B = [&](const double* v, const double* sp) {
#pragma unroll
    for (int q = 0; q < 6; q++) {
      const unsigned r = (unsigned)(rB + q);
      if (r < 64u) {
        double* d = sB + r * kLd + 3 * pj;
        double b0 = v[3 * q], b1 = v[3 * q + 1], b2 = v[3 * q + 2];
        if (q == 0) b0 += sp[0], b1 += sp[1], b2 += sp[2];
        if (q < 2 && (q == 1) == sc_opt) b0 += blv[0], b1 += blv[1], b2 += blv[2];  // (uniform) the b_l column's row
        d[0] = b0, d[1] = b1, d[2] = b2;
      }
    }
  };
  int ch = next_chunk(c0), buf = 0;
  int nx = ch < c1 ? next_chunk(ch + 1) : c1;
  int nx2 = nx < c1 ? next_chunk(nx + 1) : c1;
  int eT = -1, eB = -1;
  if (wv < 3) {
    load_blk(tab_of(aT, aTc, ch), ta);
    if (offdiag) load_blk(tab_of(aB, aBc, ch), tb);
    if (spT) load_special(aT, ch, !offdiag, spT3, blv);
    if (offdiag && spB) load_special(aB, ch, true, spB3, blv);
    eT = tab_of(aT, aTc, nx);
    if (offdiag) eB = tab_of(aB, aBc, nx);
  } else {
    load_hll(ch);
    store_dinv(0);
    load_hll(nx);
  }
  while (ch < c1) {
    __syncthreads();  // the previous chunk's fragments have been read; sDi[buf] is complete
    if (wv < 3) {
      stage_T(ta, sDi[buf] + pj * 9);
      if (offdiag)
        stage_B(tb, spB3);
      else
        stage_B(ta, spT3);
    } else {
      store_dinv(buf ^ 1);  // chunk nx, from the H_ll loaded an iteration ago
      load_hll(nx2);
    }
    __syncthreads();
    const int nx3 = nx2 < c1 ? next_chunk(nx2 + 1) : c1;
    if (wv < 3 && nx < c1) {
      load_blk(eT, ta);
      if (offdiag) load_blk(eB, tb);
      if (spT) load_special(aT, nx, !offdiag, spT3, blv);
      if (offdiag && spB) load_special(aB, nx, true, spB3, blv);
      eT = tab_of(aT, aTc, nx2);
      if (offdiag) eB = tab_of(aB, aBc, nx2);
    }
    if (!OFFDIAG) {  // (branches on nblk, not masks: v_mfma ignores EXEC)
      const int fo = (lane & 15) * kLd + (lane >> 4);
      const double *pa0 = sT + bi0 * 16 * kLd + fo, *pb0 = sB + bj0 * 16 * kLd + fo;
      const double *pa1 = sT + bi1 * 16 * kLd + fo, *pb1 = sB + bj1 * 16 * kLd + fo;
      const double *pa2 = sT + bi2 * 16 * kLd + fo, *pb2 = sB + bj2 * 16 * kLd + fo;
      if (nblk == 3) {
#pragma unroll
        for (int ks = 0; ks < 3 * kChunkLm / 4; ks++) {
          acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa0[ks * 4], pb0[ks * 4], acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa1[ks * 4], pb1[ks * 4], acc[1], 0, 0, 0);
          acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa2[ks * 4], pb2[ks * 4], acc[2], 0, 0, 0);
        }
      } else if (nblk == 2) {
#pragma unroll
        for (int ks = 0; ks < 3 * kChunkLm / 4; ks++) {
          acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa0[ks * 4], pb0[ks * 4], acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa1[ks * 4], pb1[ks * 4], acc[1], 0, 0, 0);
        }
      } else if (nblk == 1) {
#pragma unroll
        for (int ks = 0; ks < 3 * kChunkLm / 4; ks++)
          acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa0[ks * 4], pb0[ks * 4], acc[0], 0, 0, 0);
      }
    } else {
      const double* pa = sT + (wv * 16 + (lane & 15)) * kLd + (lane >> 4);
      const double* pb = sB + (lane & 15) * kLd + (lane >> 4);
#pragma unroll
      for (int ks = 0; ks < 3 * kChunkLm / 4; ks++) {
        const double av = pa[ks * 4];
        acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, pb[ks * 4], acc[0], 0, 0, 0);
#pragma unroll
        for (int q = 1; q < 4; q++)  // (the last column tile: the blocks up to column npv's)
          if (q < nq) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, pb[q * 16 * kLd + ks * 4], acc[q], 0, 0, 0);
      }
    }
    buf ^= 1, ch = nx, nx = nx2, nx2 = nx3;
  }
  // f64 C/D map: col = lane & 15, row = (lane >> 4) + 4 * reg
  double* S = D.Sp + (size_t)split * D.sp_stride;
  if (!OFFDIAG) {  // the wavefront's blocks, nothing else
    const size_t ld = TILES ? 64 : (size_t)D.ldS;
    S += TILES ? (size_t)bt * kGbaTileElems : (size_t)(bi * 64) * ld + bj * 64;
    S += (size_t)(lane >> 4) * ld + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; r++) {
      if (nblk > 0) S[(size_t)(bi0 * 16 + 4 * r) * ld + bj0 * 16] = acc[0][r];
      if (nblk > 1) S[(size_t)(bi1 * 16 + 4 * r) * ld + bj1 * 16] = acc[1][r];
      if (nblk > 2) S[(size_t)(bi2 * 16 + 4 * r) * ld + bj2 * 16] = acc[2][r];
    }
    return;
  }
  if (TILES) {
    S += (size_t)bt * kGbaTileElems;
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
      for (int r = 0; r < 4; r++)
        if (q < nq) S[(wv * 16 + (lane >> 4) + 4 * r) * 64 + q * 16 + (lane & 15)] = acc[q][r];
    return;
  }
#pragma unroll
  for (int q = 0; q < 4; q++)
#pragma unroll
    for (int r = 0; r < 4; r++)
      if (q < nq) S[(size_t)(bi * 64 + wv * 16 + (lane >> 4) + 4 * r) * D.ldS + bj * 64 + q * 16 + (lane & 15)] = acc[q][r];
}

// Landmark-sharded window: this rank's part of everything the ranks have to sum -- the
// Schur product over its landmarks (K-split partials folded in fixed order), H_pp and b_p of its edges
// -- packed contiguously for ONE all-reduce.
__global__ void __launch_bounds__(256)
k_lba_pack(const LbaDev* __restrict__ devs, const WinCtl* __restrict__ ctl) {
  const int w = blockIdx.y;
  if (!(ctl[w].flags & LBA_TRIAL)) return;
  const LbaDev& D = devs[w];
  if (!D.red) return;
  const int npv = D.npv, nS = npv * (npv + 1), nH = 36 * D.n_free, nb = 6 * D.n_free;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= nS + nH + nb + (D.scale_opt ? nb + 2 : 0)) return;
  if (e < nS) {
    const int ksplit = D.ksplit;
    const int nchunks = (D.n_mp + kChunkLm - 1) / kChunkLm, cps = (nchunks + ksplit - 1) / ksplit;
    const int ns = (nchunks + cps - 1) / cps;
    const int r = e / (npv + 1), c = e - r * (npv + 1);
    const int rr = c < npv ? min(r, c) : r, cc = c < npv ? max(r, c) : npv;
    double s = 0;
    for (int k = 0; k < ns; k++) s += D.Sp[(size_t)k * D.sp_stride + (size_t)rr * D.ldS + cc];
    D.red[e] = s;
  } else if (e < nS + nH)
    D.red[e] = D.Hpp[e - nS];
  else if (e < nS + nH + nb)
    D.red[e] = D.bp[e - nS - nH];
  else
    D.red[e] = D.sc_sys[e - nS - nH - nb];  // H_ps, H_ss, b_s of the scale vertex
}

// Reduced pose system.  PR x PR entries: Hpp + lambda I - S (both triangles from the upper block-tiles of
// the Schur partials); visual-inertial windows add the inertial edges' 30x30 blocks, gathered per entry
// (a key frame has at most one inertial edge in and one out).  bs = b - S[:, npv], bfull = b.
// The sum over the K splits of the Schur partials at (rr <= cc).  TILES: the planned tile storage (a tile outside the plan
// is a structural zero: the dense product holds +0 there, and so does this sum).
template <bool TILES>
__device__ __forceinline__ double lba_schur_sum(const LbaDev& D, int ns, int rr, int cc) {
  double s = 0;
  if (TILES) {
    const int bi = rr >> 6, bj = cc >> 6, end = D.sch_ptr[bi + 1];
    int lo = D.sch_ptr[bi], hi = end;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (D.sch_j[mid] < bj)
        lo = mid + 1;
      else
        hi = mid;
    }
    if (lo == end || D.sch_j[lo] != bj) return s;
    const double* p = D.Sp + (size_t)lo * kGbaTileElems + (rr & 63) * 64 + (cc & 63);
    for (int k = 0; k < ns; k++) s += p[(size_t)k * D.sp_stride];
  } else {  // four loads in flight, then their adds: the order k = 0 .. ns - 1 is the sum's definition
    const double* p = D.Sp + (size_t)rr * D.ldS + cc;
    const size_t st = D.sp_stride;
    int k = 0;
    for (; k + 4 <= ns; k += 4) {
      const double x0 = p[k * st], x1 = p[(k + 1) * st], x2 = p[(k + 2) * st], x3 = p[(k + 3) * st];
      s += x0, s += x1, s += x2, s += x3;
    }
    for (; k < ns; k++) s += p[k * st];
  }
  return s;
}

// A free key frame's pair edges (inertial / encoder), as the entry functions below look them up: from the window's
// tables, or from a copy of them that a solve kernel staged in LDS (five ints per free key frame: key frame, edge in,
// edge out, the out edge's far key frame, the in edge's).
struct LbaLinksDev {
  const LbaDev& D;
  __device__ __forceinline__ int kf(int a) const { return D.kf_list[a]; }
  __device__ __forceinline__ int ein(int a) const { return D.kf_in[D.kf_list[a]]; }
  __device__ __forceinline__ int eout(int a) const { return D.kf_out[D.kf_list[a]]; }
  __device__ __forceinline__ int far_out(int a, int e) const { return D.imu[e].j; }
  __device__ __forceinline__ int far_in(int a, int e) const { return D.imu[e].i; }
};
struct LbaLinksLds {
  const int* t;
  __device__ __forceinline__ int kf(int a) const { return t[5 * a]; }
  __device__ __forceinline__ int ein(int a) const { return t[5 * a + 1]; }
  __device__ __forceinline__ int eout(int a) const { return t[5 * a + 2]; }
  __device__ __forceinline__ int far_out(int a, int e) const { return t[5 * a + 3]; }
  __device__ __forceinline__ int far_in(int a, int e) const { return t[5 * a + 4]; }
};
__device__ __forceinline__ void lba_links_stage(const LbaDev& D, int a, int* t) {
  const int ka = D.kf_list[a], ein = D.kf_in[ka], eout = D.kf_out[ka];
  t[5 * a] = ka, t[5 * a + 1] = ein, t[5 * a + 2] = eout;
  t[5 * a + 3] = eout >= 0 ? D.imu[eout].j : -1, t[5 * a + 4] = ein >= 0 ? D.imu[ein].i : -1;
}

// entry (r, c) of the reduced system, c <= r's 16-block (the summation order of every entry is fixed here)
// (_at: with r = pd a + ra and c = pd b + cb split by the caller)
template <bool TILES, class LINKS>
__device__ __forceinline__ double lba_assemble_entry_at(const LbaDev& D, const LINKS& L, int r, int c, int a, int ra, int b,
                                                        int cb, double lambda, int ns) {
  const int np = D.np, npv = D.npv, pd = D.pd;
  // the scale vertex (bScaleOpt) is the last row / column; its row of the visual system is the last one as well
  const bool rs = D.scale_opt && r == np - 1, cs = D.scale_opt && c == np - 1;
  const int vr = rs ? npv - 1 : (ra < 6 ? 6 * a + ra : -1), vc = cs ? npv - 1 : (cb < 6 ? 6 * b + cb : -1);
  double v = 0;
  const double* redS = TILES ? nullptr : D.red;  // sums over the K splits and over the ranks, see k_lba_pack
  const double* redH = redS ? redS + (size_t)npv * (npv + 1) : D.Hpp;
  const double* redb = redS ? redH + 36 * (size_t)D.n_free : D.bp;
  const double* redsc = redS ? redb + 6 * (size_t)D.n_free : D.sc_sys;
  if (vr >= 0 && vc >= 0) {
    const int rr = min(vr, vc), cc = max(vr, vc);
    double s = 0;
    if (redS)
      s = redS[(size_t)rr * (npv + 1) + cc];
    else
      s = lba_schur_sum<TILES>(D, ns, rr, cc);
    v = -s;
    if (rs && cs)
      v += redsc[6 * D.n_free];  // H_ss
    else if (rs)
      v += redsc[6 * b + cb];  // H_ps^T
    else if (cs)
      v += redsc[6 * a + ra];
    else if (a == b)
      v += redH[36 * (size_t)a + ra * 6 + cb];
  }
  if ((pd == 15 || D.n_imu > 0) && !rs) {  // pair edges: inertial (+ encoder) of a 15-dim window, encoder only of a 6-dim one
    const int ein = L.ein(a), eout = L.eout(a);
    if (!cs) {
      const int kb = L.kf(b);
      if (a == b) {
        if (ein >= 0) v += D.Ae[930 * (size_t)ein + (15 + ra) * 30 + 15 + cb];
        if (eout >= 0) v += D.Ae[930 * (size_t)eout + ra * 30 + cb];
      } else {
        if (eout >= 0 && L.far_out(a, eout) == kb) v += D.Ae[930 * (size_t)eout + ra * 30 + 15 + cb];
        if (ein >= 0 && L.far_in(a, ein) == kb) v += D.Ae[930 * (size_t)ein + (15 + ra) * 30 + cb];
      }
    }
  }
  if (r == c) v += lambda;
  return v;
}
template <bool TILES>
__device__ __forceinline__ double lba_assemble_entry(const LbaDev& D, int r, int c, double lambda, int ns) {
  const int pd = D.pd, a = r / pd, b = c / pd;
  return lba_assemble_entry_at<TILES>(D, LbaLinksDev{D}, r, c, a, r - a * pd, b, c - b * pd, lambda, ns);
}

// gradient of row r: g = b (bfull), t = S[r, npv] (bs = g - t)
template <bool TILES, class LINKS>
__device__ __forceinline__ void lba_assemble_rhs_at(const LbaDev& D, const LINKS& L, int r, int a, int ra, int ns, double& g,
                                                    double& t) {
  const int np = D.np, npv = D.npv, pd = D.pd;
  const bool rs = D.scale_opt && r == np - 1;
  const int vr = rs ? npv - 1 : (ra < 6 ? 6 * a + ra : -1);
  const double* redS = TILES ? nullptr : D.red;
  const double* redH = redS ? redS + (size_t)npv * (npv + 1) : D.Hpp;
  const double* redb = redS ? redH + 36 * (size_t)D.n_free : D.bp;
  const double* redsc = redS ? redb + 6 * (size_t)D.n_free : D.sc_sys;
  g = 0, t = 0;
  if (vr >= 0) {
    g = rs ? redsc[6 * D.n_free + 1] : redb[6 * a + ra];
    if (redS)
      t = redS[(size_t)vr * (npv + 1) + npv];
    else
      t = lba_schur_sum<TILES>(D, ns, vr, npv);
  }
  if ((pd == 15 || D.n_imu > 0) && !rs) {
    const int ein = L.ein(a), eout = L.eout(a);
    if (ein >= 0) g += D.Ae[930 * (size_t)ein + 900 + 15 + ra];
    if (eout >= 0) g += D.Ae[930 * (size_t)eout + 900 + ra];
  }
}
template <bool TILES>
__device__ __forceinline__ void lba_assemble_rhs(const LbaDev& D, int r, int ns, double& g, double& t) {
  const int a = r / D.pd;
  lba_assemble_rhs_at<TILES>(D, LbaLinksDev{D}, r, a, r - a * D.pd, ns, g, t);
}

__global__ void __launch_bounds__(256)
k_lba_assemble(const LbaDev* __restrict__ devs, const WinCtl* __restrict__ ctl, const WinOut* __restrict__ out,
               const int* __restrict__ wins) {
  const int w = wins[blockIdx.y];  // the windows of one solver class: the grid is sized for that class's systems
  if (!(ctl[w].flags & LBA_TRIAL)) return;
  const LbaDev& D = devs[w];
  const int np = D.np;
  const double lambda = win_lambda(ctl[w], out[w]);
  const int ksplit = D.ksplit;
  const int nchunks = (D.n_mp + kChunkLm - 1) / kChunkLm, cps = (nchunks + ksplit - 1) / ksplit;
  const int ns = (nchunks + cps - 1) / cps;
  // (one launch per solver class, over that class's windows only: sizing one grid for the largest window of a mixed
  // batch launched 112 k workgroups of which the ordinary windows' 90 % returned at once, a small fixed grid left the
  // bLarge windows' threads nine dependent gathers each.  The solve kernels read the 16 x 16 blocks on and below the
  // diagonal only.)
  for (int e = blockIdx.x * 256 + threadIdx.x; e < np * np; e += gridDim.x * 256) {
    const int r = e / np, c = e % np;
    if ((c >> 4) > (r >> 4)) continue;
    D.Hs[e] = lba_assemble_entry<false>(D, r, c, lambda, ns);
    if (c == 0) {
      double g, t;
      lba_assemble_rhs<false>(D, r, ns, g, t);
      D.bfull[r] = g;
      D.bs[r] = g - t;
    }
  }
}

// The same entries straight into the tile pool of the tile-sparse solve (solver 3), with k_big_init's bordering: row n is
// b - S[:, npv], the padding is the identity (1e300 on row n's diagonal: it never limits a pivot).  One thread per element
// of a stored tile; the upper part of a diagonal tile is zero (never read).
__global__ void __launch_bounds__(256)
k_lba_assemble_tiles(const LbaDev* __restrict__ devs, const WinCtl* __restrict__ ctl, const WinOut* __restrict__ out,
                     const int* __restrict__ wins) {
  const int w = wins[blockIdx.y];
  if (!(ctl[w].flags & LBA_TRIAL)) return;
  const LbaDev& D = devs[w];
  if (D.solver != 3) return;
  const int n = D.np;
  if (blockIdx.x == 0 && threadIdx.x == 0) *D.big_fail = 0;
  if (n == 0) return;
  const double lambda = win_lambda(ctl[w], out[w]);
  const int ksplit = D.ksplit;
  const int nchunks = (D.n_mp + kChunkLm - 1) / kChunkLm, cps = (nchunks + ksplit - 1) / ksplit;
  const int ns = (nchunks + cps - 1) / cps;
  const size_t total = (size_t)D.n_tiles * kGbaTileElems;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int t = (int)(e / kGbaTileElems), q = (int)(e % kGbaTileElems);
    const int r = D.tile_i[t] * 64 + (q >> 6), c = D.tile_j[t] * 64 + (q & 63);
    double v = r == c ? (r == n ? 1e300 : 1.0) : 0.0;
    if (c > r)
      v = 0.0;
    else if (r < n) {
      v = lba_assemble_entry<true>(D, r, c, lambda, ns);
      if (c == r) {
        double g, tt;
        lba_assemble_rhs<true>(D, r, ns, g, tt);
        D.bfull[r] = g;
        D.bs[r] = g - tt;
      }
    } else if (r == n && c < n) {
      double g, tt;
      lba_assemble_rhs<true>(D, c, ns, g, tt);
      v = g - tt;
    }
    D.Hb[e] = v;
  }
}

}  // namespace vieo
