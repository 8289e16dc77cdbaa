// lba.hip -- Optimizer::LocalBundleAdjustment on gfx950 (reference: src/Optimizer.cc:1876-2307;
// g2o BlockSolver<6,3> with Schur complement, block_solver.hpp:353-589; LM
// optimization_algorithm_levenberg.cpp:61-207; edges src/Odom/g2otypes.h:321-547).
//
// Several independent windows advance in lock step; every kernel covers all windows of the batch
// (grid y / x = window) and returns at once for windows whose control word does not ask for the step.
// Device side (all FP64, no floating-point atomics: every sum has a fixed order, so a window's result
// does not depend on what it is batched with):
//   k_lba_begin      initializeOptimization(): active key frames / points from the edge levels, the
//                    reduced-system column of every free key frame, the (free kf, point) -> edge table
//   k_lba_error      edge-parallel residuals + robust chi2 (per-block partial sums)
//   k_lba_build      buildSystem: one thread per point over its observations (H_ll, b_l); one
//                    workgroup per free key frame over its edge list (H_pp, b_p) which also writes the
//                    6 x 3 blocks B = Jp^T W Jx of its edges, COMPACT: one 144-byte block per observation
//                    (CB[edge]); `tab` maps (free key frame, point) to the edge that carries the block
//   k_lba_lambda     computeLambdaInit (tau * max diagonal) for windows starting an optimize()
//   k_lba_schur      the Schur complement as what it is, a GEMM: (BB D^-1) x [BB; b_l]^T with
//                    D = blockdiag(H_ll + lambda I), K = 3 x points split over workgroups, 64x64 output
//                    tiles on the FP64 matrix cores (v_mfma_f64_16x16x4_f64); the dense operand tiles exist
//                    only in LDS: a K-chunk is staged from the compact blocks through `tab` (zeros where a key
//                    frame does not see a point), D^-1 applied on the way; per-split partial products
//   k_lba_assemble   Hs = H_pp + lambda I - sum of the partials (fixed order), bs likewise: for the systems of 160
//                    unknowns and more (k_lba_ldltg, k_big_*); k_lba_ldlt16 forms its own through the same functions
//   k_lba_ldlt16     one workgroup per window: the reduced system formed in LDS (no Hs), its blocked LDL^T (FP64
//                    MFMA), solve, pose retraction (with backup) and the pose part of the gain-ratio scale
//   k_lba_ldltg      the same left-looking, the factor in L2 as 16 x 16 blocks, for systems of 160 .. 639 unknowns
//   k_big_*          the tiled LDL^T over many workgroups beyond that (full BA), dense or over the stored tiles of the
//                    symbolic fill pattern (gba_sparse_plan.h)
//   k_lba_update_points  back-substitution x_l = D^-1 (b_l - B^T x_p), point update (with backup)
//   k_lba_restore / k_lba_classify  rejected-step rollback; chi2 / depth gates
// The Levenberg-Marquardt policy (lambda, accept / reject, termination, stop flag) runs on the host
// exactly as g2o's does, from one WinOut record per window and round (lba_policy.h).
//
// Full BA with bScaleOpt (System::FinalGBA, src/System.cc:24-33; Optimizer.cc:842-851,1131-1137,1190-1196,1256-1335):
// the VertexScale (g2otypes.h:292-311) is one more 1-dim column at the END of the pose system and the visual edges are
// EdgeReprojectPRS / PRSStereo (g2otypes.h:321-541, MODE_OPT_VAR == 1): Xw = s Xh, J_s = (Jproj Rcw) Xh,
// J_Xh = s (Jproj Rcw).  The scale sees every point, so it is one more (dense) row of BB -- row 6 x free key frames --
// and the Schur GEMM, the pack / all-reduce and the solves take it like any other row; its own blocks (H_ss, b_s,
// H_ps) are summed in fixed order by k_lba_build / k_lba_scale_fold and gathered by lba_assemble_entry_at.
#include <atomic>
#include <chrono>
#include <mutex>
#include <thread>
#include <vector>

#include "gba_sparse_plan.h"
#include "imu_device.h"
#include "lba_policy.h"
#include "rccl_dl.h"

namespace vieo {

struct LbaKf {
  double p[3], qw, qx, qy, qz;
  int col;    // offset of the key frame's block in the reduced pose system, -1 = fixed / inactive
  int fixed;
  double v[3], dbg[3], dba[3], bg[3], ba[3];  // visual-inertial windows (a18) only
};

// one key-frame pair of a visual-inertial window: EdgeNavStatePRV + EdgeNavStateBias
struct LbaImu {
  int i, j;          // key frames (kf_i = previous)
  int has_imu, robust;
  double InfoI[81];  // Sigma_PRV^-1, x 1e-2 when kf_i is fixed (Optimizer.cc:247-259)
  double infoBg, infoBa;
  vieo_imu_preint M;
  int has_enc, enc_robust;  // EdgeEncNavStatePR of the pair (Optimizer.cc:323-347)
  double measE[6], InfoE[36];
};

static const int kBuildChunk = 512;  // edges of a key frame per run (= workgroup) of k_lba_build's key-frame half (2 per thread)

struct LbaDev {
  const vieo_lba_obs* obs;
  int n_obs, n_mp, n_kf, nf_cap;  // nf_cap: non-fixed key frames = rows of `tab`
  int np, n_free, npv;            // written by k_lba_begin: np = pd * n_free, npv = 6 * n_free
  int pd;                         // reduced-system dims per free key frame: 6 (PR) or 15 (PR + V + Bias)
  int n_imu;
  const LbaImu* imu;              // [n_imu]
  const int *kf_in, *kf_out;      // [n_kf] inertial edge ending / starting at the key frame, -1 = none
  double* Ae;                     // [n_imu][930] generic Hessian 30x30 + gradient 30, local order
                                  //   [kf_i: PR V Bias | kf_j: PR V Bias]
  double *gchi0, *gchi;           // [n_imu] robust chi2 of the inertial edges (at linearisation / after a trial)
  double* bfull;                  // [np] gradient of the pose block (visual + inertial)
  double* red;                    // landmark-sharded window: [S npv x (npv+1) | Hpp | bp], summed over the ranks
  double* red_sc;                 //   and its scalars [chi0, chi2, scale_l, pad]
  const unsigned char* close;     // [n_mp] bClose flags or null
  double thMono, thMonoClose, thStereo;  // chi2 gates of the classification
  double gw[3];
  double th_dist_far;             // > 0: the far-point rule of the visual-inertial local BA is on
  double qRbe[4], pbe[3];         // body <- encoder extrinsics of the encoder edges
  int ldS;                        // leading dimension of a partial Schur product
  int* kf_list;                   // [n_free] free + active key frames in column order
  int* kf_act;                    // [n_kf] scratch of k_lba_begin: the key frame has an active edge
  const int *kf_edge_first, *kf_edge_idx;  // edges grouped by key frame
  int* tab;                       // [nf_cap][n_mp] edge of (free kf ordinal, point), -1 = none
  LbaKf *kf, *kf_bak;
  PoseXf* xf;                     // [n_kf][max(1, n_cams)] the key frames' transforms per camera at the CURRENT states: written
                                  // where the states change (k_lba_prelevel(0) / k_lba_begin, lba_apply_step, k_lba_restore),
                                  // read by every visual edge
  double *X, *X_bak;              // [n_mp][3]
  double* err;                    // [n_obs][3]
  unsigned char *level, *erase, *mp_act;
  const int *mp_first, *mp_count;  // [n_mp]
  double* CB;                     // [n_obs][18] B = Jp^T W Jx of an edge (6 x 3, row-major); valid where `tab` points
  double* Bs;                     // [n_mp][3] the scale vertex's row (bScaleOpt): it sees every point
  double* Sp;                     // [ksplit][sp_rows][ldS] partial Schur products
  size_t sp_stride;
  int ksplit;                     // K splits of this window's Schur GEMM (a function of the window alone)
  double *Hll, *bl, *Hpp, *bp, *Hs, *bs, *xp;
  unsigned char* occ;             // [(npv + 64) / 64][chunks of 16 landmarks]: the row tile has an edge in the chunk
  int use_occ;                    // full BA only: a local window is dense at that granularity, its Schur GEMM does not look
  double *Hb, *Wp;                // tiled solve of a large reduced system: padded copy [nb][nb], panel [nb][64]
  int* big_fail;                  //   and its "not positive definite" flag
  int nb;
  double *part0, *part, *part_m, *pmax;  // per-block partials
  double* part_t;                 // [blocks of 64 points] robust chi2 of a trial, summed per point block (k_lba_tail)
  int* tail_cnt;                  // arrival counter of k_lba_tail's workgroups (the last one folds the partials)
  // key-frame half of k_lba_build: a key frame's edge list in chunks of kBuildChunk edges, one workgroup each
  int n_chunks;                   // written by k_lba_begin: chunks of the free + active key frames
  int fold_kernel;                // batches: the runs' sums are added by k_lba_build_fold, not by the last workgroup to arrive
                                  // (its device-scope fence, an L2 write-back per workgroup on this multi-XCD part, cost a
                                  // 205-window step 3.2 -> 13.6 ms of k_lba_build)
  int *chunk_first, *chunk_kf;    // [n_free + 1] first chunk of kf_list[a]; [n_chunks] the a of a chunk
  int* chunk_cnt;                 // [n_free] arrival counters (the last workgroup of a key frame folds its chunks' partials)
  double* chunk_part;             // [n_chunks][33] H_pp (21) + b_p (6) + H_ps (6) of a chunk
  CamD cam;                       // the single rectified pinhole camera (n_cams == 0) ...
  CamD cams[4];                   // ... or the physical cameras of a distorted multi-camera rig
  int n_cams;
  const unsigned char* ocam;      // [n_obs] camera of every observation (n_cams > 0)
  double dMono, dStereo;
  int solver;                     // which solve kernel owns the window in a mixed batch (solver_class): 0 blocked LDS
                                  // (<= 159 unknowns), 1 left-looking 16 x 16 blocks (<= 639), 2 tiled multi-workgroup
                                  // LDL^T, 3 the same over the stored tiles of the fill pattern
  int scale_opt;                  // bScaleOpt: the VertexScale is the last column of the pose system
  double* scl;                    // [2] VertexScale estimate, its backup (push / pop)
  double* sc_sys;                 // [6 nf_cap + 2] H_ps per free key frame (Jp^T W Js), then H_ss, b_s
  double* psc;                    // [blocks of 64 points][2] partial sums of H_ss, b_s
  // tile-sparse LDL^T (solver 3, full BA; gba_sparse_plan.h): Sp holds the planned Schur tiles [ksplit][tile][64][64]
  // (sp_stride = tiles x 4096), Hb the tile pool (a slot per stored tile of the bordered lower triangle), Wp [nt 64][64]
  const int *sch_ptr, *sch_i, *sch_j, *sch_diag, *sch_off;  // Schur tiles row by row; the diagonal / off-diagonal ones
  int n_sch_diag, n_sch_off;
  const int *col_ptr, *tile_i, *tile_j;  // stored tiles column by column (diagonal first): slot -> (row, column) tile
  const int *row_ptr, *row_j, *row_tile;  // the same row by row (column ascending, diagonal last): column tile, slot
  const int *upd_ptr, *upd;              // panel k's update targets: (i, j, slot ik, slot jk, slot ij)
  int nt, n_tiles;
};

__device__ __forceinline__ double win_scale(const LbaDev& D) { return D.scale_opt ? D.scl[0] : 1.0; }
// s * Xh: the point the edges project (g2otypes.h:376; s == 1 without the scale vertex)
__device__ __forceinline__ void scaled_point(const LbaDev& D, int m, double* Xs) {
  const double s = win_scale(D);
  Xs[0] = D.X[3 * (size_t)m] * s, Xs[1] = D.X[3 * (size_t)m + 1] * s, Xs[2] = D.X[3 * (size_t)m + 2] * s;
}

__device__ __forceinline__ const CamD& obs_cam(const LbaDev& D, int i) { return D.n_cams ? D.cams[D.ocam[i]] : D.cam; }

__device__ __forceinline__ void kf_xf(const CamD& c, const LbaKf& k, PoseXf& X) {
  Est e;
  e.p[0] = k.p[0], e.p[1] = k.p[1], e.p[2] = k.p[2];
  e.qw = k.qw, e.qx = k.qx, e.qy = k.qy, e.qz = k.qz;
  make_xf(c, e, X);
}

// The transform table.  An entry is make_xf of the key frame's state and the camera, the very values an edge would
// compute for itself, formed once per state change instead of once per edge and pass.
__device__ __forceinline__ int xf_cams(const LbaDev& D) { return D.n_cams ? D.n_cams : 1; }
__device__ __forceinline__ const PoseXf& obs_xf(const LbaDev& D, int i, int kf) {
  return D.xf[(size_t)kf * xf_cams(D) + (D.n_cams ? D.ocam[i] : 0)];
}
__device__ __forceinline__ void write_kf_xf(const LbaDev& D, int k, const LbaKf& kf) {
  // (formed in registers, then stored: the stores may alias the descriptor as far as the compiler knows, and writing
  //  through make_xf had k_lba_begin re-load the camera between them)
  PoseXf X;
  if (D.n_cams)
    for (int c = 0; c < D.n_cams; c++) {
      kf_xf(D.cams[c], kf, X);
      D.xf[(size_t)k * D.n_cams + c] = X;
    }
  else {
    kf_xf(D.cam, kf, X);
    D.xf[k] = X;
  }
}

// residual with a double-precision point (the LBA point vertex is double, unlike PoseOpt's)
__device__ __forceinline__ double lba_edge_error(const CamD& c, const PoseXf& X, const vieo_lba_obs& o,
                                                 const double* Xw, double* err, double* Pc) {
  for (int i = 0; i < 3; i++)
    Pc[i] = X.Rcw[i * 3] * Xw[0] + X.Rcw[i * 3 + 1] * Xw[1] + X.Rcw[i * 3 + 2] * Xw[2] + X.tcw[i];
  double uv[2];
  cam_project(c, Pc, uv, nullptr);
  const double u = uv[0], v = uv[1];
  err[0] = (double)o.u - u;
  err[1] = (double)o.v - v;
  const double info = (double)o.inv_sigma2;
  double chi2 = err[0] * (info * err[0]) + err[1] * (info * err[1]);
  if (o.ur >= 0) {
    err[2] = (double)o.ur - (u - c.bf / Pc[2]);
    chi2 += err[2] * (info * err[2]);
  } else
    err[2] = 0;
  return chi2;
}

// Jp (3x6) and Jx (3x3) of one edge
__device__ __forceinline__ void lba_jacobians(const CamD& c, const PoseXf& X, const double* kfp,
                                              const double* Xw, const double* Pc, double* Jp, double* Jx) {
  const double invz = 1 / Pc[2], invz2 = invz * invz;
  double J[9], Jc[6], uv[2];
  cam_project(c, Pc, uv, Jc);  // Jproj = -d(u, v)/dPc (g2otypes.h:453-459)
  J[0] = -Jc[0], J[1] = -Jc[1], J[2] = -Jc[2];
  J[3] = -Jc[3], J[4] = -Jc[4], J[5] = -Jc[5];
  J[6] = J[0], J[7] = J[1], J[8] = J[2] - c.bf * invz2;
  const double d0 = Xw[0] - kfp[0], d1 = Xw[1] - kfp[1], d2 = Xw[2] - kfp[2];
  double Pa[3], RH[9];
  for (int m = 0; m < 3; m++) Pa[m] = X.Rwb[m] * d0 + X.Rwb[3 + m] * d1 + X.Rwb[6 + m] * d2;
  for (int m = 0; m < 3; m++) {
    const double a = c.Rcb[m * 3], b = c.Rcb[m * 3 + 1], d = c.Rcb[m * 3 + 2];
    RH[m * 3 + 0] = b * Pa[2] - d * Pa[1];
    RH[m * 3 + 1] = -a * Pa[2] + d * Pa[0];
    RH[m * 3 + 2] = a * Pa[1] - b * Pa[0];
  }
  for (int r = 0; r < 3; r++)
    for (int q = 0; q < 3; q++) {
      Jp[r * 6 + q] = -(J[r * 3] * c.Rcb[q] + J[r * 3 + 1] * c.Rcb[3 + q] + J[r * 3 + 2] * c.Rcb[6 + q]);
      Jp[r * 6 + 3 + q] = J[r * 3] * RH[q] + J[r * 3 + 1] * RH[3 + q] + J[r * 3 + 2] * RH[6 + q];
      Jx[r * 3 + q] = J[r * 3] * X.Rcw[q] + J[r * 3 + 1] * X.Rcw[3 + q] + J[r * 3 + 2] * X.Rcw[6 + q];
    }
}


__device__ __forceinline__ double win_lambda(const WinCtl& c, const WinOut& o) {
  return c.lambda >= 0 ? c.lambda : o.lambda;
}

// (H_ll + lambda I)^-1 of one landmark
__device__ __forceinline__ void landmark_dinv(const double* H, double lambda, double* Di) {
  const double a00 = H[0] + lambda, a01 = H[1], a02 = H[2], a10 = H[3], a11 = H[4] + lambda, a12 = H[5],
               a20 = H[6], a21 = H[7], a22 = H[8] + lambda;
  const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
  const double id = 1.0 / (a00 * c00 + a01 * c01 + a02 * c02);
  Di[0] = c00 * id, Di[1] = (a02 * a21 - a01 * a22) * id, Di[2] = (a01 * a12 - a02 * a11) * id;
  Di[3] = c01 * id, Di[4] = (a00 * a22 - a02 * a20) * id, Di[5] = (a02 * a10 - a00 * a12) * id;
  Di[6] = c02 * id, Di[7] = (a01 * a20 - a00 * a21) * id, Di[8] = (a00 * a11 - a01 * a10) * id;
}

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
__device__ __forceinline__ void lba_generic_dev(const LbaDev& D, int e, int lane, int mode);
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

// ---- inertial edges of a visual-inertial window: one wavefront per key-frame pair.
// mode 0: linearise at the current state (30x30 block J^T (rho' Omega) J and gradient, both edges of the
// pair) and robust chi2 -> gchi0; mode 1: robust chi2 after a trial -> gchi.
// (the body, for one wavefront: k_lba_generic's workgroups and the pair workgroups of k_lba_tail)
__device__ __forceinline__ void lba_generic_dev(const LbaDev& D, int e, int lane, int mode) {
  __shared__ double sJ[9 * 30], sT[9 * 30], sErr[9 + 6], sWe[9], sRho[3];
  __shared__ double sJE[6 * 30], sTE[6 * 30], sWeE[6];  // encoder edge: J in the local order, (rho' Info) J, Info e
  // the edge's record staged in LDS by the whole wavefront: lane 0's chains below read it field by field, and every
  // dependent batch of those reads was a trip to L2
  static_assert(sizeof(LbaImu) % 8 == 0, "staged in 8-byte words");
  __shared__ __align__(16) double sE_store[sizeof(LbaImu) / 8];
  {
    const double* src = reinterpret_cast<const double*>(&D.imu[e]);
    for (int i = lane; i < (int)(sizeof(LbaImu) / 8); i += 64) sE_store[i] = src[i];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  const LbaImu& E = *reinterpret_cast<const LbaImu*>(sE_store);
  const double dI = (double)(float)sqrt(16.919), dB = (double)(float)sqrt(12.592);  // Optimizer.cc:219-222
  if (lane == 0) {
    NSd si, sj;
    const LbaKf &ki = D.kf[E.i], &kj = D.kf[E.j];
    for (int k = 0; k < 3; k++) {
      si.p[k] = ki.p[k], si.v[k] = ki.v[k], si.bg[k] = ki.bg[k], si.ba[k] = ki.ba[k];
      si.dbg[k] = ki.dbg[k], si.dba[k] = ki.dba[k];
      sj.p[k] = kj.p[k], sj.v[k] = kj.v[k], sj.bg[k] = kj.bg[k], sj.ba[k] = kj.ba[k];
      sj.dbg[k] = kj.dbg[k], sj.dba[k] = kj.dba[k];
    }
    si.qw = ki.qw, si.qx = ki.qx, si.qy = ki.qy, si.qz = ki.qz;
    sj.qw = kj.qw, sj.qx = kj.qx, sj.qy = kj.qy, sj.qz = kj.qz;
    double chi = 0, rI = 1.0, rB = 1.0;
    if (E.has_imu) {
      imu_error(E.M, D.gw, si, sj, sErr, 3);
      double c2 = 0;
      for (int a = 0; a < 9; a++) {
        double t = 0;
        for (int b = 0; b < 9; b++) t += E.InfoI[a * 9 + b] * sErr[b];
        sWe[a] = t;
        c2 += sErr[a] * t;
      }
      double r0 = c2;
      if (E.robust) huber(c2, dI, dI * dI, &r0, &rI);
      chi += r0;
    }
    for (int k = 0; k < 3; k++) {
      sErr[9 + k] = (sj.bg[k] + sj.dbg[k]) - (si.bg[k] + si.dbg[k]);
      sErr[12 + k] = (sj.ba[k] + sj.dba[k]) - (si.ba[k] + si.dba[k]);
    }
    {
      double c2 = 0;
      for (int k = 0; k < 3; k++) c2 += sErr[9 + k] * (E.infoBg * sErr[9 + k]);
      for (int k = 3; k < 6; k++) c2 += sErr[9 + k] * (E.infoBa * sErr[9 + k]);
      double r0 = c2;
      if (E.robust) huber(c2, dB, dB * dB, &r0, &rB);
      chi += r0;
    }
    double rE = 1.0;
    if (E.has_enc) {
      double errE[6], JEi[36], JEj[36];
      enc_edge_eval(si, sj, E.measE, D.qRbe, D.pbe, errE, mode == 0 ? JEi : nullptr, mode == 0 ? JEj : nullptr);
      double c2 = 0;
      for (int a = 0; a < 6; a++) {
        double t = 0;
        for (int b = 0; b < 6; b++) t += E.InfoE[a * 6 + b] * errE[b];
        sWeE[a] = t;
        c2 += errE[a] * t;
      }
      double r0 = c2;
      if (E.enc_robust) huber(c2, dB, dB * dB, &r0, &rE);  // sqrt(12.592), Optimizer.cc:343
      chi += r0;
      if (mode == 0)
        for (int a = 0; a < 6; a++) {
          for (int c = 0; c < 30; c++) sJE[a * 30 + c] = 0;
          for (int c = 0; c < 6; c++) sJE[a * 30 + c] = JEi[a * 6 + c], sJE[a * 30 + 15 + c] = JEj[a * 6 + c];
        }
    }
    (mode ? D.gchi : D.gchi0)[e] = chi;
    sRho[0] = rI, sRho[1] = rB, sRho[2] = rE;
    if (mode == 0 && E.has_imu) {
      // J (9 x 24, [PRV_j | PRV_i | Bias_i]) -> local order [i: PR V Bias | j: PR V Bias]
      double* J24 = sT;  // (LDS, free until the products below: as a local array it lived in scratch, 1.7 KB per lane)
      imu_linearize(E.M, D.gw, si, sj, sErr, J24, 3, 6);
      for (int a = 0; a < 9; a++) {
        for (int c = 0; c < 30; c++) sJ[a * 30 + c] = 0;
        for (int c = 0; c < 9; c++) sJ[a * 30 + 15 + c] = J24[a * 24 + c];       // state j: PR, V
        for (int c = 0; c < 9; c++) sJ[a * 30 + c] = J24[a * 24 + 9 + c];        // state i: PR, V
        for (int c = 0; c < 6; c++) sJ[a * 30 + 9 + c] = J24[a * 24 + 18 + c];   // Bias_i
      }
    }
  }
  if (mode) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  double* A = D.Ae + 930 * (size_t)e;
  const double rI = sRho[0], rB = sRho[1], rE = sRho[2];
  if (E.has_enc) {
    for (int t = lane; t < 180; t += 64) {
      const int a = t / 30, c = t - a * 30;
      double u = 0;
      for (int q = 0; q < 6; q++) u += (rE * E.InfoE[a * 6 + q]) * sJE[q * 30 + c];
      sTE[t] = u;
    }
  }
  if (E.has_imu) {
    for (int t = lane; t < 270; t += 64) {  // T = (rho' Info) J
      const int a = t / 30, c = t - a * 30;
      double u = 0;
      for (int q = 0; q < 9; q++) u += (rI * E.InfoI[a * 9 + q]) * sJ[q * 30 + c];
      sT[t] = u;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  for (int t = lane; t < 900; t += 64) {
    const int c1 = t / 30, c2 = t - c1 * 30;
    double u = 0;
    if (E.has_imu)
      for (int a = 0; a < 9; a++) u += sJ[a * 30 + c1] * sT[a * 30 + c2];
    if (E.has_enc)
      for (int a = 0; a < 6; a++) u += sJE[a * 30 + c1] * sTE[a * 30 + c2];
    // bias edge: J_i = -I on rows/cols 9..14, J_j = +I on 24..29
    const int b1 = c1 >= 24 ? c1 - 24 : (c1 >= 9 && c1 < 15 ? c1 - 9 : -1);
    const int b2 = c2 >= 24 ? c2 - 24 : (c2 >= 9 && c2 < 15 ? c2 - 9 : -1);
    if (b1 >= 0 && b1 == b2) {
      const double wgt = (b1 < 3 ? E.infoBg : E.infoBa) * rB;
      u += ((c1 >= 24) == (c2 >= 24)) ? wgt : -wgt;
    }
    A[t] = u;
  }
  if (lane < 30) {
    double u = 0;
    if (E.has_imu)
      for (int a = 0; a < 9; a++) u += sJ[a * 30 + lane] * (-sWe[a] * rI);
    if (E.has_enc)
      for (int a = 0; a < 6; a++) u += sJE[a * 30 + lane] * (-sWeE[a] * rE);
    const int b1 = lane >= 24 ? lane - 24 : (lane >= 9 && lane < 15 ? lane - 9 : -1);
    if (b1 >= 0) {
      const double we = (b1 < 3 ? E.infoBg : E.infoBa) * sErr[9 + b1] * rB;
      u += lane >= 24 ? -we : we;
    }
    A[900 + lane] = u;
  }
}
__global__ void __launch_bounds__(64)
k_lba_generic(const LbaDev* __restrict__ devs, const WinCtl* __restrict__ ctl, int mode) {
  const int w = blockIdx.y, fl = ctl[w].flags;
  if (!(fl & (mode ? LBA_TRIAL : LBA_BUILD))) return;
  const LbaDev& D = devs[w];
  if ((int)blockIdx.x >= D.n_imu) return;
  lba_generic_dev(D, blockIdx.x, threadIdx.x, mode);
}

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

// ================================================================== host-side lock-step LM driver
static thread_local hipStream_t g_lba_stream = nullptr;
static thread_local int g_lba_stream_dev = -1;  // the device the stream was created on
static thread_local int g_lba_priority = -2;    // vieo_lba_set_stream_priority of this host thread (-2: VIEO_LBA_PRIORITY / -1)
static thread_local DevBuf g_arena, g_small;
static thread_local PinnedBuf g_stage, g_small_h;

struct WinHost {  // a window of a call on the host
  const vieo_lba_params* P;
  const vieo_lba_vio_params* VP = nullptr;  // visual-inertial window (a18)
  const vieo_lba_enc* ENC = nullptr;        // encoder edges of a vision-only window (a17)
  int n_kf, n_mp, n_obs, n_imu = 0;
  int nf = 0;  // free key frames
  bool skip = false;   // takes no part in the rounds: no free pose, or the stop flag was up at entry
  int cls = 0;         // solver_class of its reduced system
  GbaSparsePlan plan;  // class 3: the symbolic plan of the tile-sparse solve
  WinLm lm;            // its LM state machine (lba_policy.h)
  size_t o_kf, o_X, o_erase, o_scl;  // offsets of the results in the staging buffer (plan_window)
};

// n x n inverse (n <= 9) by Gauss-Jordan with partial pivoting: the 9 x 9 pre-integration covariance
// (GetProcessedInfoijPRV: mSigmaijPRV.inverse()), the 6 x 6 encoder covariance
static bool inverse_n(const double* A, double* Ainv, int n) {
  double M[9][18];
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) M[i][j] = A[i * n + j], M[i][n + j] = (i == j);
  for (int c = 0; c < n; c++) {
    int piv = c;
    for (int r = c + 1; r < n; r++)
      if (std::fabs(M[r][c]) > std::fabs(M[piv][c])) piv = r;
    if (M[piv][c] == 0) return false;
    if (piv != c)
      for (int j = 0; j < 2 * n; j++) std::swap(M[c][j], M[piv][j]);
    const double d = M[c][c];
    for (int j = 0; j < 2 * n; j++) M[c][j] /= d;
    for (int r = 0; r < n; r++)
      if (r != c) {
        const double f = M[r][c];
        if (f != 0)
          for (int j = 0; j < 2 * n; j++) M[r][j] -= f * M[c][j];
      }
  }
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) Ainv[i * n + j] = M[i][n + j];
  return true;
}

struct LbaShard {  // landmark-sharded run: every rank holds all key frames and its share of the points
  vieo_allreduce_sum_f64_fn fn;
  void* ctx;
  double* d_buf;
  size_t cap;
};

// one exchange of a sharded run: the caller's callback (complete on return; the stream is drained first) or, with
// fn == nullptr, ncclAllReduce on the stream itself (ctx = the communicator of vieo_rccl_comm_create)
static int shard_exchange(const LbaShard* sh, double* d_buf, size_t n, hipStream_t st) {
  if (sh->fn) {
    VIEO_HIP_CHECK(hipStreamSynchronize(st));
    if (sh->fn(sh->ctx, d_buf, n) != 0) {
      set_error("sharded local BA: the all-reduce callback failed");
      return VIEO_E_INVALID;
    }
    return VIEO_OK;
  }
  return rccl_allreduce_sum_f64(sh->ctx, d_buf, n, st);
}

// All ranks of a sharded run agree on go / no-go: the sum of the ranks' failure flags through the run's own exchange.
// Every rank must call it the same number of times.  *sum > 0: some rank failed.
// stop / *stop_any: the ranks' stop requests travel in the same number (4096 per request: exact in a double for any
// realistic job size), so that pbStopFlag raised on one rank aborts the call on all of them together.
static int shard_agree(const LbaShard* sh, bool ok, double* sum, bool stop = false, bool* stop_any = nullptr) {
  const double flag = (ok ? 0.0 : 1.0) + (stop ? 4096.0 : 0.0);
  *sum = 1.0;
  VIEO_HIP_CHECK(hipMemcpy(sh->d_buf, &flag, 8, hipMemcpyHostToDevice));
  const int xrc = shard_exchange(sh, sh->d_buf, 1, nullptr);
  if (xrc != VIEO_OK) return xrc;
  VIEO_HIP_CHECK(hipStreamSynchronize(nullptr));
  double total = 0;
  VIEO_HIP_CHECK(hipMemcpy(&total, sh->d_buf, 8, hipMemcpyDeviceToHost));
  const double stops = std::floor(total / 4096.0);
  if (stop_any) *stop_any = stops > 0;
  *sum = total - 4096.0 * stops;
  return VIEO_OK;
}

// A rank that leaves lba_run between the first agreement and the rounds (a staging error only it ran into: allocation
// failure, a singular covariance) still takes part in the second agreement -- with a failure flag -- so that the
// other ranks return too instead of waiting for it in the first all-reduce of the rounds.
struct ShardStagingGuard {
  const LbaShard* sh;
  bool done = false;
  ~ShardStagingGuard() {
    if (sh && !done) {
      double sum;
      (void)shard_agree(sh, false, &sum);
    }
  }
};

// packed reduced visual system of a window with nf free key frames (k_lba_pack); sc: with the scale vertex's row,
// H_ps, H_ss, b_s
static size_t shard_sys_doubles(int nf, int sc = 0) {
  const size_t nv = (size_t)6 * nf + (sc ? 1 : 0);
  return nv * (nv + 1) + 36 * (size_t)nf + 6 * (size_t)nf + (sc ? 6 * (size_t)nf + 2 : 0);
}

// reduced systems beyond one workgroup's LDL^T take the tiled solve (VIEO_LBA_BIG_SOLVE=1 forces it: tests)
static const int kSmallSolveMax = 16 * kLdGMaxBlocks - 1, kBigSolveMax = 16320;
// ---- optional kernel-class timing (vieo_lba_enable_timing): HIP events around every launch on the BA stream, folded
// into process-wide totals after each round's synchronisation.  bench.py reads them for the roofline of the whole path.
enum LbaKClass { KC_BUILD, KC_GENERIC, KC_SCHUR, KC_ASSEMBLE, KC_LDLT, KC_UPDATE, KC_ERROR, KC_BEGIN, KC_OTHER, KC_LDLT_SPARSE, KC_N };
static const char* const kLbaKClassName[KC_N] = {"lba.build", "lba.generic", "lba.schur", "lba.assemble", "lba.ldlt",
                                                 "lba.update_points", "lba.error", "lba.begin", "lba.other",
                                                 "lba.ldlt_sparse"};
static std::atomic<int> g_lba_ktiming{0};
static std::mutex g_lba_kt_mutex;
static double g_lba_kt_ms[KC_N];
static long long g_lba_kt_launches[KC_N];
static double g_lba_kt_schur_flops;  // dense FLOPs of the timed k_lba_schur launches
// the last tile-sparse call of this process (vieo_lba_sparse_stats): stored tiles, tiles of the dense lower triangle,
// planned Schur tiles, planned upper Schur tiles of the dense grid, plan bytes, arena bytes
static long long g_lba_sparse_stats[6];

struct LbaKTimer {
  bool on = false, count_only = false;  // count_only (mode 2): launches per class without events
  hipStream_t st = nullptr;
  std::vector<hipEvent_t> pool;
  std::vector<int> cls;  // class of pair i (events 2i, 2i + 1)
  void begin(hipStream_t s) {
    const int mode = g_lba_ktiming.load();
    on = mode != 0, count_only = mode == 2;
    st = s;
    cls.clear();
  }
  template <class F>
  void launch(int c, F&& f) {
    if (!on) {
      f();
      return;
    }
    if (count_only) {
      f();
      cls.push_back(c);
      return;
    }
    const size_t i = cls.size();
    while (pool.size() < 2 * (i + 1)) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) {
        on = false;
        f();
        return;
      }
      pool.push_back(e);
    }
    (void)hipEventRecord(pool[2 * i], st);
    f();
    (void)hipEventRecord(pool[2 * i + 1], st);
    cls.push_back(c);
  }
  void fold(double schur_flops_per_launch) {  // after the stream was synchronised
    if (!on || cls.empty()) return;
    std::lock_guard<std::mutex> g(g_lba_kt_mutex);
    bool schur_seen = false;  // a round's Schur complement is two launches (diagonal / off-diagonal tiles): FLOPs once
    for (size_t i = 0; i < cls.size(); i++) {
      float ms = 0;
      if (!count_only && hipEventElapsedTime(&ms, pool[2 * i], pool[2 * i + 1]) != hipSuccess) continue;
      g_lba_kt_ms[cls[i]] += ms, g_lba_kt_launches[cls[i]]++;
      if (cls[i] == KC_SCHUR && !schur_seen) g_lba_kt_schur_flops += schur_flops_per_launch, schur_seen = true;
    }
    cls.clear();
  }
};

static bool big_solve(int n) {
  static const int forced = [] {
    const char* e = getenv("VIEO_LBA_BIG_SOLVE");
    return e ? atoi(e) : 0;
  }();
  return forced > 0 || n > kSmallSolveMax;
}

static bool sparse_solve_forced() {  // VIEO_LBA_SPARSE_SOLVE=1: every full BA takes the tile-sparse solve (tests)
  static const int forced = [] {
    const char* e = getenv("VIEO_LBA_SPARSE_SOLVE");
    return e ? atoi(e) : 0;
  }();
  return forced > 0;
}

// The solve kernel of a window with n unknowns.  Windows of different classes share a lock-step batch: every class's
// kernel is launched (when one of its windows takes a trial this round) and skips the others' windows (a bLarge
// window of 25 key frames next to ordinary ones of 10 is the usual LocalMapping mix).
//   0  k_lba_ldlt16   n <= 159: blocked on the matrix cores, whole triangle in LDS
//   1  k_lba_ldltg    n <= 639: one workgroup, left-looking, the factor in L2 as column-major 16 x 16 blocks
//   2  k_big_*        the tiled LDL^T over many workgroups (full BA: hundreds of key frames)
//   3  k_big_*<TILES> the same over the stored tiles of the symbolic fill pattern (gba_sparse_plan.h): the full BA
//                     (full_ba: not landmark-sharded) beyond kBigSolveMax unknowns, or any with VIEO_LBA_SPARSE_SOLVE=1
static int solver_class(int n, bool full_ba = false) {
  if (full_ba && (sparse_solve_forced() || n > kBigSolveMax)) return 3;
  if (big_solve(n)) return 2;
  if (((n + 16) >> 4) <= kLd16MaxBlocks) return 0;
  return 1;
}

// Optimizer::BundleAdjustment / GlobalBundleAdjustmentNavStatePRV (Optimizer.cc:1353-1609, 771-1345) on the same
// engine: ONE optimize(iterations), Huber kernels on every edge iff `robust`, no chi2 classification, no
// Chi2LargeSetLevel, g2o's own initial lambda, no divergence guard.
struct GbaMode {
  int iterations, robust;
  int scale_opt = 0;          // bScaleOpt (System::FinalGBA): VertexScale + EdgeReprojectPRS[Stereo]
  double* scale_out = nullptr;  // the recovered scale (1 when the call returns early)
};

// Observation i of a window: sorted by map point, key-frame, camera and map-point indices in range, distorted
// observations monocular (nc: the window's n_cams).
static bool lba_obs_ok(const vieo_lba_obs* ob, int i, int n_mp, int n_kf, int nc) {
  const int kfi = ob[i].kf & 0xFFFFFF, ci = (ob[i].kf >> 24) & 15;
  return !(ob[i].mp < 0 || ob[i].mp >= n_mp || ob[i].kf < 0 || kfi >= n_kf || (i > 0 && ob[i].mp < ob[i - 1].mp) ||
           (nc == 0 ? ci != 0 : (ci >= nc || ob[i].ur >= 0)));
}
static int lba_obs_invalid() {
  set_error("vieo_local_bundle_adjustment: observations must be sorted by map point, key frame and camera indices in "
            "range, distorted observations monocular");
  return VIEO_E_INVALID;
}


// One call of the engine, as every bundle-adjustment entry of the C-ABI states it.  vparams == nullptr ->
// Optimizer::LocalBundleAdjustment (params, encs), otherwise LocalBundleAdjustmentNavStatePRV (vparams, h_close, h_imu,
// n_imu).  gba != nullptr: the full BA of the same kind.  sh != nullptr: this process is one rank of a landmark-sharded
// run.
struct LbaCall {
  const LbaShard* sh = nullptr;
  const GbaMode* gba = nullptr;
  int W = 0;  // windows
  const vieo_lba_params* const* params = nullptr;
  const vieo_lba_vio_params* const* vparams = nullptr;
  const vieo_lba_keyframe* const* h_kfs = nullptr;
  const float* const* h_points = nullptr;
  const uint8_t* const* h_close = nullptr;
  const vieo_lba_obs* const* h_obs = nullptr;
  const vieo_lba_imu_edge* const* h_imu = nullptr;
  const int *n_kf = nullptr, *n_mp = nullptr, *n_obs = nullptr, *n_imu = nullptr;  // per window
  volatile const int* stop = nullptr;
  vieo_navstate* const* h_navs_out = nullptr;
  float* const* h_points_out = nullptr;
  uint8_t* const* h_erase = nullptr;
  vieo_lba_result* h_results = nullptr;
  const vieo_lba_enc* const* encs = nullptr;  // EdgeEncNavStatePR of vision-only windows (Optimizer.cc:2008-2042, 1401-1438)

  bool vio() const { return vparams != nullptr; }
  int pd() const { return vio() ? 15 : 6; }  // reduced-system dims per free key frame
  int sco() const { return gba && gba->scale_opt ? 1 : 0; }
  bool stop_raised() const { return stop && *stop; }
  LmMode lm_mode() const { return LmMode{gba != nullptr, gba && gba->robust != 0, vio() && !gba}; }
};

// The argument checks of lba_run, without side effects: VIEO_OK or the error code, with its text.  A landmark-sharded
// run calls it first and lets all ranks agree on the outcome with one all-reduce: a rank that returned early on its own
// while the others were already waiting in the collective would hang them.  A rank of a sharded run may own no point
// (or no observation) of a window.  The observations of an unsharded call are checked while the staging threads copy
// them (fill_window): a pass of its own over them, on one thread, cost 0.3 ms per bench step.
static int lba_check_args(const LbaCall& c) {
  const bool vio = c.vio(), sharded = c.sh != nullptr;
  const int pd = c.pd(), sco = c.sco();
  if (c.W <= 0 || (!vio && !c.params) || !c.h_kfs || !c.n_kf || !c.h_points || !c.n_mp || !c.h_obs || !c.n_obs ||
      !c.h_navs_out || !c.h_points_out || !c.h_erase || !c.h_results || (vio && (!c.h_close || !c.h_imu || !c.n_imu))) {
    set_error("bundle adjustment: a missing argument or no window");
    return VIEO_E_INVALID;
  }
  for (int w = 0; w < c.W; w++) {
    const vieo_lba_params* P = vio ? (c.vparams[w] ? &c.vparams[w]->base : nullptr) : c.params[w];
    const vieo_lba_enc* enc = !vio && c.encs ? c.encs[w] : nullptr;
    const int n_kf = c.n_kf[w], n_mp = c.n_mp[w], n_obs = c.n_obs[w];
    if (!P || !c.h_kfs[w] || n_kf <= 0 || n_mp < 0 || n_obs < 0 || !c.h_navs_out[w] ||
        (!sharded && (n_mp == 0 || n_obs == 0)) || (n_mp > 0 && (!c.h_points[w] || !c.h_points_out[w])) ||
        (n_obs > 0 && (!c.h_obs[w] || !c.h_erase[w])) ||
        (vio && ((!c.h_close[w] && !c.gba) || c.n_imu[w] < 0 || (c.n_imu[w] > 0 && !c.h_imu[w]))) ||
        (enc && (enc->n_edges < 0 || (enc->n_edges > 0 && !enc->edges)))) {
      set_error("bundle adjustment: window %d has a missing buffer or a bad count", w);
      return VIEO_E_INVALID;
    }
    int nf = 0;
    for (int k = 0; k < n_kf; k++) nf += !c.h_kfs[w][k].fixed;
    // (the full BA's tile-sparse solve has no such limit: its device memory is checked once the arena is laid out)
    if (((!c.gba || sharded) && pd * nf + sco > kBigSolveMax) || n_kf >= (1 << 24)) {
      set_error("bundle adjustment: %d free key frames exceed the reduced-system limit of %d unknowns", nf, kBigSolveMax);
      return VIEO_E_CAPACITY;
    }
    const int ne = vio ? c.n_imu[w] : enc ? enc->n_edges : 0;
    std::vector<char> in(n_kf, 0), outk(n_kf, 0);
    for (int t = 0; t < ne; t++) {  // a chain: at most one pre-integration into and one out of every key frame
      const int a = vio ? c.h_imu[w][t].kf_i : enc->edges[t].kf_i, b = vio ? c.h_imu[w][t].kf_j : enc->edges[t].kf_j;
      if (a < 0 || a >= n_kf || b < 0 || b >= n_kf || a == b || outk[a] || in[b]) {
        set_error("local BA: the inertial / encoder edges must chain the key frames");
        return VIEO_E_INVALID;
      }
      outk[a] = 1, in[b] = 1;
    }
    const int nc = P->n_cams;
    if (nc < 0 || nc > 4 || (nc > 0 && !P->cams)) {
      set_error("local BA: n_cams must be 0..4");
      return VIEO_E_INVALID;
    }
    for (int ci = 0; ci < nc; ci++) {
      const vieo_camera& cam = P->cams[ci];
      if (cam.model < 0 || cam.model > 2 || (cam.model == VIEO_CAM_RADTAN && (cam.num_k < 2 || cam.num_k > 6))) {
        set_error("local BA: camera %d has an unknown model or coefficient count", ci);
        return VIEO_E_INVALID;
      }
    }
    for (int i = 0; sharded && i < n_obs; i++)
      if (!lba_obs_ok(c.h_obs[w], i, n_mp, n_kf, nc)) return lba_obs_invalid();
  }
  return VIEO_OK;
}

// Check the call; the ranks of a sharded run agree on the outcome (first agreement) and on the stop flag.
// (configuration errors, the same on every rank of a job; `stop` is rank-local and asynchronous: a sharded run never
// acts on its own copy -- the ranks' requests are summed in the exchanges the run makes anyway (the two agreements
// at entry, the fourth scalar of every trial), so all ranks take the abort at the same point: Optimizer.cc:524-528,570-571)
static int lba_check_and_agree(const LbaCall& c, bool* shard_stop) {
  const LbaShard* sh = c.sh;
  if (sh && (!c.vio() || (!sh->fn && !sh->ctx) || !sh->d_buf)) {
    set_error("sharded local BA: visual-inertial windows only, with a reduction callback and buffer");
    return VIEO_E_INVALID;
  }
  const int rc = require_device();  // (a rank without a device cannot take part in the job at all)
  if (rc != VIEO_OK) return rc;
  if (!sh) return lba_check_args(c);
  // every rank reaches this collective whatever its own arguments look like; the sum of the failure flags decides
  // for all of them
  const bool ok = sh->cap >= 1 && lba_check_args(c) == VIEO_OK;
  double sum = 1.0;
  if (sh->cap >= 1) {
    const int xrc = shard_agree(sh, ok, &sum, c.stop_raised(), shard_stop);
    if (xrc != VIEO_OK) return xrc;
  }
  if (sum != 0.0) {
    set_error(ok ? "sharded local BA: another rank rejected its arguments, all ranks return"
                 : "sharded local BA: invalid arguments on this rank (all ranks return)");
    return VIEO_E_INVALID;
  }
  return VIEO_OK;
}

// This host thread's bundle-adjustment stream on the current device.
static int lba_stream(hipStream_t* st) {
  int cur = 0;
  (void)hipGetDevice(&cur);
  if (g_lba_stream && g_lba_stream_dev != cur) g_lba_stream = nullptr;  // the thread moved to another GPU
  g_lba_stream_dev = cur;
  if (!g_lba_stream) {
    // VIEO_LBA_PRIORITY = -1 / 0 / 1: lowest / default / highest stream priority for the bundle-adjustment stream.
    // Lowest by default: local mapping is the background thread of the reference and tracking must not wait for
    // it.  Next to a batched front end on another stream the bench step measured (30 steps, 205 windows per step):
    // highest 48.9 k frames/s with k_fast at 9.3 ms per launch and 0.17 ms per window; default 50.1 k / 7.6 / 0.79;
    // lowest 53.0 k / 7.7 (what k_fast takes alone) / 0.73 -- the windows' kernels are short and many and fill what the
    // front end leaves free instead of taking CUs from it.
    // One window beside a tracker is the other case: the sequential replay measured 1.03 ms per frame with the stream at
    // the DEFAULT priority against 1.08 at the lowest and 1.07 at the highest (the solve finishes sooner and the tracker
    // waits less for its write-back): the LocalMapping thread of such a host asks for it with vieo_lba_set_stream_priority(0).
    int lo = 0, hi = 0;
    const char* e = getenv("VIEO_LBA_PRIORITY");
    const int want = g_lba_priority != -2 ? g_lba_priority : (e ? atoi(e) : -1);
    if (want == 0 || hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess || lo == hi)
      VIEO_HIP_CHECK(hipStreamCreateWithFlags(&g_lba_stream, hipStreamNonBlocking));
    else
      VIEO_HIP_CHECK(hipStreamCreateWithPriority(&g_lba_stream, hipStreamNonBlocking, want < 0 ? lo : hi));
  }
  *st = g_lba_stream;
  return VIEO_OK;
}

// The windows of a call: counts, outputs preset to the inputs, which of them take part (stopped: the stop flag was up
// at entry), the solver class of those and the symbolic plan of the tile-sparse solve (built once: the full BA never
// reclassifies its edges).  Returns how many take part.
static int lba_open_windows(const LbaCall& c, bool stopped, std::vector<WinHost>& win) {
  const bool vio = c.vio();
  const int pd = c.pd(), sco = c.sco();
  const LmMode mode = c.lm_mode();
  int n_live = 0;
  for (int w = 0; w < c.W; w++) {
    WinHost& H = win[w];
    if (vio)
      H.VP = c.vparams[w], H.P = &c.vparams[w]->base, H.n_imu = c.n_imu[w];
    else {
      H.P = c.params[w];
      if (c.encs && c.encs[w]) H.ENC = c.encs[w], H.n_imu = c.encs[w]->n_edges;
    }
    H.n_kf = c.n_kf[w], H.n_mp = c.n_mp[w], H.n_obs = c.n_obs[w];  // (a rank of a sharded run may own no point of a window)
    const vieo_lba_keyframe* kfs = c.h_kfs[w];
    for (int k = 0; k < H.n_kf; k++) H.nf += !kfs[k].fixed;
    memset(&c.h_results[w], 0, sizeof(vieo_lba_result));
    lm_start(H.lm, mode, c.gba ? c.gba->iterations : H.P->its0, H.P->its1, vio ? H.VP->lambda_init : 0.0, &c.h_results[w]);
    for (int k = 0; k < H.n_kf; k++) c.h_navs_out[w][k] = kfs[k].nav;
    if (H.n_mp > 0) memcpy(c.h_points_out[w], c.h_points[w], (size_t)H.n_mp * 12);
    if (H.n_obs > 0) memset(c.h_erase[w], 0, H.n_obs);
    if (!H.nf && !sco)  // (bdimPoses = true with the scale vertex: Optimizer.cc:850)
      H.skip = true, lm_skip(H.lm, VIEO_LBA_NO_FREE_POSE);  // Optimizer.cc:1993
    else if (stopped)
      H.skip = true, lm_skip(H.lm, VIEO_LBA_ABORTED);
    if (H.skip) continue;
    n_live++;
    H.cls = solver_class(pd * H.nf + sco, c.gba && !c.sh);
    if (H.cls != 3) continue;
    std::vector<int> fx(H.n_kf), okf(H.n_obs), omp(H.n_obs), pi(H.n_imu), pj(H.n_imu);
    for (int k = 0; k < H.n_kf; k++) fx[k] = kfs[k].fixed;
    for (int i = 0; i < H.n_obs; i++) okf[i] = c.h_obs[w][i].kf, omp[i] = c.h_obs[w][i].mp;
    for (int t = 0; t < H.n_imu; t++) {
      pi[t] = vio ? c.h_imu[w][t].kf_i : H.ENC->edges[t].kf_i;
      pj[t] = vio ? c.h_imu[w][t].kf_j : H.ENC->edges[t].kf_j;
    }
    gba_sparse_plan(H.plan, H.n_kf, fx.data(), H.n_obs, okf.data(), omp.data(), H.n_mp, H.n_imu, pi.data(), pj.data(), pd, sco);
  }
  return n_live;
}

// ---- the device arena: [inputs | results (kf, X, erase, scale) | zero-initialised | scratch], the windows interleaved
// inside every region, every buffer rounded to 256 bytes.  plan_window names each buffer once -- region, the LbaDev
// pointer it feeds (whose type is its element type) and its element count; arena_layout gives them their offsets and
// arena_bind turns the offsets into pointers once a base is known (the pinned staging copy, then the device arena).
enum { R_IN, R_RES, R_ZERO, R_SCR, R_N };
struct ArenaItem {
  size_t bytes;
  bool absent;   // the window has no such buffer: the pointer is the arena's base, never dereferenced
  void* field;   // the pointer it feeds
  size_t* keep;  // where the host keeps the offset (WinHost: the results it reads back), or null
  size_t off;
};
struct WinArena {
  std::vector<ArenaItem> region[R_N];
  const int* plan = nullptr;  // the tile-sparse solve's lists (solver 3), one block in plan_lists() order
  template <class T>
  void add(int r, T*& field, size_t count, size_t* keep = nullptr) {
    region[r].push_back({count * sizeof(T), false, (void*)&field, keep, 0});
  }
  template <class T>
  void none(int r, T*& field) {
    region[r].push_back({0, true, (void*)&field, nullptr, 0});
  }
};
struct LbaLayout {
  std::vector<WinArena> win;
  size_t arena = 0, res_begin = 0, res_end = 0, zero_end = 0;  // total bytes; where the regions meet
};

// the plan's lists as the device reads them: (vector, where its pointer goes in LbaDev)
static std::vector<std::pair<const std::vector<int>*, const int**>> plan_lists(const GbaSparsePlan& P, LbaDev* D) {
  return {{&P.sch_ptr, &D->sch_ptr}, {&P.sch_i, &D->sch_i}, {&P.sch_j, &D->sch_j}, {&P.sch_diag, &D->sch_diag},
          {&P.sch_off, &D->sch_off}, {&P.col_ptr, &D->col_ptr}, {&P.tile_i, &D->tile_i}, {&P.tile_j, &D->tile_j},
          {&P.row_ptr, &D->row_ptr}, {&P.row_j, &D->row_j}, {&P.row_tile, &D->row_tile}, {&P.upd_ptr, &D->upd_ptr},
          {&P.upd, &D->upd}};
}

static void arena_layout(LbaLayout& L) {
  size_t* const ends[R_N] = {&L.res_begin, &L.res_end, &L.zero_end, &L.arena};
  for (int r = 0; r < R_N; r++) {
    for (WinArena& A : L.win)
      for (ArenaItem& it : A.region[r]) {
        if (it.absent) continue;
        it.off = L.arena;
        L.arena += (it.bytes + 255) / 256 * 256;
        if (it.keep) *it.keep = it.off;
      }
    *ends[r] = L.arena;
  }
}

// the pointers of regions [r0, r1) of a window against `base`
static void arena_bind(WinArena& A, const WinHost& H, LbaDev& D, int r0, int r1, uint8_t* base) {
  for (int r = r0; r < r1; r++)
    for (const ArenaItem& it : A.region[r]) {
      uint8_t* p = base + it.off;
      memcpy(it.field, &p, sizeof(p));
    }
  if (r0 == R_IN && H.cls == 3) {
    const int* d = A.plan;
    for (auto& l : plan_lists(H.plan, &D)) *l.second = d, d += l.first->size();
  }
}

// Schur GEMM decomposition: 64x64 block-tiles (upper) x K splits.  The number of splits is a function of the window
// alone (about 8 chunks of 16 landmarks per workgroup, cps_target), so that the summation order -- and with it the
// window's result -- does not depend on what the window is batched with; a mixed batch (ordinary windows of one
// tile next to bLarge ones of six) launches the largest tile x split count and the others' workgroups exit.
// Measured per call of 205 windows, cps_target = 3 / 6 / 12 / 24: Schur 4.9 / 4.6 / 4.7 / 6.1 ms, k_lba_assemble
// (which sums the partials) 2.1 / 1.6 / 1.2 / 1.1 ms.  The full BA keeps few splits: its tiles are many and
// mostly skipped (k_lba_occ).
static int schur_tiles(int npm) {  // npm: rows of the visual system
  const int RB = (npm + 63) / 64, CB = (npm + 64) / 64;
  return RB * CB - RB * (RB - 1) / 2;
}
static int schur_ksplit(int npm, int nmp, bool gba) {
  const int cps_target = 8;
  const int nch = (nmp + kChunkLm - 1) / kChunkLm, nbt = std::max(1, schur_tiles(npm));
  if (gba) return std::max(1, std::min(std::min(nch, 16), 768 / nbt));
  return std::max(1, std::min(std::min((nch + cps_target - 1) / cps_target, 32), std::max(1, 512 / nbt)));
}

// The launch grids and class tables of a batch, computed once: every kernel covers all windows of the batch, so each
// grid is the largest any window needs.
struct LbaGrids {
  int ge = 1, gm = 1, gq = 1, gr = 1;  // blocks of 256 edges / 256 points / 64 points / max(256 points, 256 key frames)
  int schur = 0, schur_off = 0;        // Schur GEMM: diagonal / off-diagonal tiles x splits of the dense windows
  int schur_t = 0, schur_t_off = 0;    //   the same over the planned tiles of the tile-sparse windows
  int cls_max[4] = {0, 0, 0, 0};       // per solver class: the largest system of the class (0: the class is empty)
  int cls_first[5] = {0, 0, 0, 0, 0};  // cls_order[cls_first[c] .. cls_first[c + 1]): the windows of class c
  std::vector<int> cls_order;          // (alive until the call returns: its copy to the device is asynchronous)
  int nb16 = 0, nbg = 0;               // 16 x 16 blocks of the largest class-0 / class-1 system
  // the tile-sparse solve: tile rows, the assembly's elements; per panel k the rows under the diagonal tile and the
  // update targets
  int sp_nt = 0;
  size_t sp_elems = 0;
  std::vector<int> sp_panel_grid, sp_syrk_grid;
  int occ_max = 0, max_chunks = 1, max_imu = 0, max_nf = 0, max_mp = 0;
  bool any_multicam = false;
  // k_lba_tail (one launch for the tail of a trial) for calls of a few windows: one window beside the tracker 5.0 -> 4.9 ms,
  // W = 4 equal, but W = 16 / 64 windows 2.80 -> 3.02 / 5.07 -> 6.47 ms per call -- its residual pass runs four lanes per
  // point over the point's edges (that is what makes it independent of the other workgroups), which is latency-bound and
  // loses to k_lba_error's lane per edge once the launch ramps are amortised over many windows.  Batches take the
  // four-launch form (the tail without the fold + k_lba_reduce over its partials measured 3.9 against 2.9 ms of kernel
  // time per 205-window step).  Both halves of k_lba_build in one launch: calls of a few windows as well.
  bool fused_tail = false, fused_build = false;
  size_t shard_sys = 0;  // sharded run: doubles of the windows' packed reduced systems in the reduction buffer
};

// A window's descriptor (everything but the arena pointers) and its rows of the arena table.
static void plan_window(const LbaCall& c, WinHost& H, LbaDev& D, WinArena& A, LbaGrids& G) {
  const bool vio = c.vio(), gba = c.gba != nullptr, tiles = H.cls == 3;
  const int sco = c.sco(), pd = c.pd(), nf = H.nf;
  const int npm = 6 * nf + sco;   // rows of the visual system: PR blocks (+ the scale vertex)
  const int npf = pd * nf + sco;  // full reduced system
  const int sp_rows = (npm + 63) / 64 * 64, ldS = (npm + 64) / 64 * 64;
  const int ksplit = schur_ksplit(npm, H.n_mp, gba);  // (the tile-sparse solve keeps the dense split: the same sums)
  const GbaSparsePlan& PL = H.plan;
  const size_t n_obs = H.n_obs, n_mp = H.n_mp, n_kf = H.n_kf, n_edge = std::max(H.n_imu, 1);
  const size_t blk256 = (n_obs + 255) / 256, blk64 = (n_mp + 63) / 64;
  // chunks of the key frames' edge lists: sum over the free key frames of ceil(edges / kBuildChunk) <= this bound
  const size_t nchk = n_obs / kBuildChunk + nf + 1;
  memset(&D, 0, sizeof(D));
  A.region[R_IN].reserve(11), A.region[R_RES].reserve(4), A.region[R_ZERO].reserve(2), A.region[R_SCR].reserve(40);
  D.nb = (npf + 1 + kNB - 1) / kNB * kNB;  // + the right-hand-side row
  if (H.cls == 1) D.nb = (npf + 16) >> 4;  // 16 x 16 blocks of the bordered matrix

  A.add(R_IN, D.obs, n_obs);
  A.add(R_IN, D.mp_first, n_mp), A.add(R_IN, D.mp_count, n_mp);
  A.add(R_IN, D.kf_edge_first, n_kf + 1), A.add(R_IN, D.kf_edge_idx, n_obs);
  A.add(R_IN, D.ocam, n_obs);
  if (vio || H.ENC) {
    A.add(R_IN, D.imu, n_edge);
    A.add(R_IN, D.kf_in, n_kf), A.add(R_IN, D.kf_out, n_kf), A.add(R_IN, D.close, n_mp);
  }
  if (tiles) A.add(R_IN, A.plan, PL.list_ints());

  A.add(R_RES, D.kf, n_kf, &H.o_kf), A.add(R_RES, D.X, 3 * n_mp, &H.o_X), A.add(R_RES, D.erase, n_obs, &H.o_erase);
  A.add(R_RES, D.scl, 2, &H.o_scl);

  A.add(R_ZERO, D.level, n_obs), A.add(R_ZERO, D.err, 3 * n_obs);

  A.add(R_SCR, D.kf_bak, n_kf), A.add(R_SCR, D.X_bak, 3 * n_mp);
  A.add(R_SCR, D.xf, n_kf * (size_t)std::max(1, H.P->n_cams));
  A.add(R_SCR, D.mp_act, n_mp);
  A.add(R_SCR, D.CB, (n_obs + 1) * 18);  // + the zero block
  if (sco)
    A.add(R_SCR, D.Bs, 3 * std::max<size_t>(n_mp, 1));
  else
    A.none(R_SCR, D.Bs);
  A.add(R_SCR, D.Sp, tiles ? PL.schur_bytes(ksplit) / 8 : (size_t)ksplit * sp_rows * ldS);
  A.add(R_SCR, D.Hll, 9 * n_mp), A.add(R_SCR, D.bl, 3 * n_mp);
  A.add(R_SCR, D.Hpp, (size_t)std::max(nf, 1) * 36);
  if (tiles) {  // no dense Hs; the tile pool, W of a panel for every row
    A.none(R_SCR, D.Hs);
    A.add(R_SCR, D.Hb, PL.pool_bytes() / 8), A.add(R_SCR, D.Wp, PL.panel_bytes() / 8), A.add(R_SCR, D.big_fail, 64);
  } else {
    if (H.cls == 0)  // formed in the solve's LDS
      A.none(R_SCR, D.Hs);
    else
      A.add(R_SCR, D.Hs, (size_t)npf * npf);
    if (H.cls == 2)
      A.add(R_SCR, D.Hb, (size_t)D.nb * D.nb), A.add(R_SCR, D.Wp, (size_t)D.nb * kNB), A.add(R_SCR, D.big_fail, 64);
    else if (H.cls == 1)
      A.add(R_SCR, D.Hb, ldg_scratch_doubles(D.nb)), A.none(R_SCR, D.Wp), A.none(R_SCR, D.big_fail);
    else
      A.none(R_SCR, D.Hb), A.none(R_SCR, D.Wp), A.none(R_SCR, D.big_fail);
  }
  A.add(R_SCR, D.bp, npm), A.add(R_SCR, D.bs, npf), A.add(R_SCR, D.xp, npf);
  A.add(R_SCR, D.bfull, npf);
  A.add(R_SCR, D.Ae, n_edge * 930);
  A.add(R_SCR, D.gchi0, n_edge), A.add(R_SCR, D.gchi, n_edge);
  A.add(R_SCR, D.part0, blk256), A.add(R_SCR, D.part, blk256);
  A.add(R_SCR, D.part_m, blk64), A.add(R_SCR, D.pmax, blk64);
  A.add(R_SCR, D.part_t, std::max<size_t>(blk64, 1)), A.add(R_SCR, D.tail_cnt, 64);
  A.add(R_SCR, D.chunk_first, nf + 1), A.add(R_SCR, D.chunk_cnt, nf + 1);
  A.add(R_SCR, D.chunk_kf, nchk), A.add(R_SCR, D.chunk_part, nchk * 33);
  A.add(R_SCR, D.kf_list, n_kf), A.add(R_SCR, D.tab, (size_t)std::max(nf, 1) * n_mp);
  A.add(R_SCR, D.sc_sys, 6 * nf + 2), A.add(R_SCR, D.psc, blk64 * 2);
  A.add(R_SCR, D.kf_act, n_kf);
  A.add(R_SCR, D.occ, (size_t)((npm + 64) / 64) * ((n_mp + kChunkLm - 1) / kChunkLm));

  D.n_obs = H.n_obs, D.n_mp = H.n_mp, D.n_kf = H.n_kf, D.nf_cap = nf;
  D.ldS = ldS, D.sp_stride = tiles ? PL.n_sch_tiles() * kGbaTileElems : (size_t)sp_rows * ldS, D.ksplit = ksplit;
  D.cam.fx = H.P->fx, D.cam.fy = H.P->fy, D.cam.cx = H.P->cx, D.cam.cy = H.P->cy, D.cam.bf = H.P->bf;
  memcpy(D.cam.Rcb, H.P->Rcb, 72);
  memcpy(D.cam.tcb, H.P->tcb, 24);
  D.n_cams = H.P->n_cams;
  for (int ci = 0; ci < H.P->n_cams; ci++) {
    const vieo_camera& cam = H.P->cams[ci];
    CamD& d = D.cams[ci];
    d.fx = cam.fx, d.fy = cam.fy, d.cx = cam.cx, d.cy = cam.cy, d.bf = 0;
    memcpy(d.Rcb, cam.Rcb, 72), memcpy(d.tcb, cam.tcb, 24);
    d.model = cam.model, d.num_k = cam.model == VIEO_CAM_RADTAN ? cam.num_k : 0;
    for (int q = 0; q < 8; q++) d.k[q] = (double)cam.dist[q];
  }
  // thHuberMono = sqrt(5.991) in the local BAs, thHuber2D = sqrt(5.99) in the global ones (Optimizer.cc:1063,1445)
  D.dMono = (double)(float)sqrt(gba ? 5.99 : 5.991), D.dStereo = (double)(float)sqrt(7.815);
  D.pd = pd, D.n_imu = H.n_imu;
  D.scale_opt = sco;
  D.use_occ = gba ? 1 : 0;
  D.solver = H.cls;
  D.fold_kernel = c.W <= 4 ? 0 : 1;
  if (tiles) {
    D.n_sch_diag = (int)PL.sch_diag.size(), D.n_sch_off = (int)PL.sch_off.size();
    D.nt = PL.nt, D.n_tiles = (int)PL.n_tiles();
  }
  if (vio) {  // const float chi2Mono = 5.991; 1.5 * chi2Mono; literal 7.815 (Optimizer.cc:347,603-620)
    D.thMono = (double)5.991f, D.thMonoClose = 1.5 * (double)5.991f, D.thStereo = 7.815;
    memcpy(D.gw, H.VP->gw, 24);
    memcpy(D.qRbe, H.VP->qRbe, 32), memcpy(D.pbe, H.VP->pbe, 24);
    D.th_dist_far = (!gba && H.VP->th_dist_far > 0 && std::isfinite(H.VP->th_dist_far)) ? (double)H.VP->th_dist_far : 0.0;
  } else {
    D.thMono = D.thMonoClose = 5.991, D.thStereo = 7.815;
    if (H.ENC) memcpy(D.qRbe, H.ENC->qRbe, 32), memcpy(D.pbe, H.ENC->pbe, 24);
  }

  // the window's share of the batch's grids
  if (tiles) {
    G.schur_t = std::max(G.schur_t, (int)PL.sch_diag.size() * ksplit);
    G.schur_t_off = std::max(G.schur_t_off, (int)PL.sch_off.size() * ksplit);
    G.sp_nt = std::max(G.sp_nt, PL.nt), G.sp_elems = std::max(G.sp_elems, PL.n_tiles() * kGbaTileElems);
    G.sp_panel_grid.resize(G.sp_nt, 1), G.sp_syrk_grid.resize(G.sp_nt, 0);
    for (int k = 0; k < PL.nt; k++) {
      G.sp_panel_grid[k] = std::max(G.sp_panel_grid[k], 1 + ((PL.col_ptr[k + 1] - PL.col_ptr[k] - 1) * kNB + 255) / 256);
      G.sp_syrk_grid[k] = std::max(G.sp_syrk_grid[k], PL.upd_ptr[k + 1] - PL.upd_ptr[k]);
    }
  } else {
    const int RBw = (npm + 63) / 64;
    G.schur = std::max(G.schur, RBw * ksplit);
    G.schur_off = std::max(G.schur_off, (schur_tiles(npm) - RBw) * ksplit);
  }
  // (at least one workgroup each: an empty landmark shard still launches everything)
  G.ge = std::max(G.ge, (H.n_obs + 255) / 256), G.gm = std::max(G.gm, (H.n_mp + 255) / 256);
  G.gq = std::max(G.gq, (H.n_mp + 63) / 64), G.gr = std::max(std::max(G.gr, G.gm), (H.n_kf + 255) / 256);
  G.max_chunks = std::max(G.max_chunks, (int)nchk), G.max_imu = std::max(G.max_imu, H.n_imu);
  G.max_nf = std::max(G.max_nf, nf), G.max_mp = std::max(G.max_mp, H.n_mp);
  G.any_multicam |= H.P->n_cams > 0;
  G.cls_max[H.cls] = std::max(G.cls_max[H.cls], npf);
}

// Descriptors, arena table and grids of the windows that take part; the offsets of everything.
static void lba_layout(const LbaCall& c, std::vector<WinHost>& win, std::vector<LbaDev>& devs, LbaLayout& L, LbaGrids& G) {
  const int W = c.W;
  L.win.resize(W);
  for (int w = 0; w < W; w++)
    if (!win[w].skip) plan_window(c, win[w], devs[w], L.win[w], G);
  arena_layout(L);
  G.occ_max = ((6 * G.max_nf + c.sco() + 64) / 64) * ((G.max_mp + kChunkLm - 1) / kChunkLm);
  for (int cl = 0; cl < 4; cl++) {
    G.cls_first[cl] = (int)G.cls_order.size();
    for (int w = 0; w < W; w++)
      if (!win[w].skip && win[w].cls == cl) G.cls_order.push_back(w);
  }
  G.cls_first[4] = (int)G.cls_order.size();
  G.nb16 = (G.cls_max[0] + 16) >> 4, G.nbg = (G.cls_max[1] + 16) >> 4;
  G.fused_tail = G.fused_build = W <= 4;
}

template <class T>
static T* staged(const T* p) {  // a descriptor bound to the staging copy: the host fills what the device will only read
  return const_cast<T*>(p);
}

// the encoder half of a key-frame pair's edge (EdgeEncNavStatePR): measurement and information, x 1e-2 when kf_i is fixed
// (Optimizer.cc:323-347, 2030-2033); d.measE / d.InfoE are zero on entry
static bool fill_enc_edge(LbaImu& d, const vieo_enc_preint& enc, bool fixed_i, int robust) {
  d.has_enc = enc.dt != 0, d.enc_robust = robust;
  if (!d.has_enc) return true;
  memcpy(d.measE, enc.delx, 48);
  if (!inverse_n(enc.Sigma, d.InfoE, 6)) return false;
  if (fixed_i)
    for (int q = 0; q < 36; q++) d.InfoE[q] *= 1e-2;
  return true;
}

// kf_in / kf_out: the pair edge ending / starting at every key frame, -1 = none
static void fill_chain(const LbaDev& S, const WinHost& H) {
  const LbaImu* im = S.imu;
  int *kin = staged(S.kf_in), *kout = staged(S.kf_out);
  for (int k = 0; k < H.n_kf; k++) kin[k] = kout[k] = -1;
  for (int t = 0; t < H.n_imu; t++) kout[im[t].i] = t, kin[im[t].j] = t;
}

// The inputs of window w into the pinned copy of the arena (index structures, key frames, inertial / encoder edges with
// their information matrices, points).  S: the window's descriptor with its input and result pointers bound to that copy.
static int fill_window(const LbaCall& c, int w, const WinHost& H, const LbaDev& S) {
  const vieo_lba_obs* ob = c.h_obs[w];
  const vieo_lba_keyframe* kfs = c.h_kfs[w];
  const int enc_robust = c.gba ? c.gba->robust != 0 : 1;
  {  // the device sees plain key-frame indices; the camera index travels in its own byte array
    vieo_lba_obs* so = staged(S.obs);
    uint8_t* ocam = staged(S.ocam);
    for (int i = 0; i < H.n_obs; i++) {
      if (!lba_obs_ok(ob, i, H.n_mp, H.n_kf, H.P->n_cams)) return lba_obs_invalid();
      so[i] = ob[i];
      so[i].kf = ob[i].kf & 0xFFFFFF;
      ocam[i] = (uint8_t)((ob[i].kf >> 24) & 15);
    }
    ob = so;
  }
  int *mp_first = staged(S.mp_first), *mp_count = staged(S.mp_count);
  int *kf_first = staged(S.kf_edge_first), *kf_idx = staged(S.kf_edge_idx);
  memset(mp_first, 0, (size_t)H.n_mp * 4), memset(mp_count, 0, (size_t)H.n_mp * 4);
  memset(kf_first, 0, (size_t)(H.n_kf + 1) * 4);
  for (int i = 0; i < H.n_obs; i++) {
    const int m = ob[i].mp;
    if (mp_count[m] == 0) mp_first[m] = i;
    mp_count[m]++;
    kf_first[ob[i].kf + 1]++;
  }
  for (int k = 0; k < H.n_kf; k++) kf_first[k + 1] += kf_first[k];
  std::vector<int> fill(kf_first, kf_first + H.n_kf);
  for (int i = 0; i < H.n_obs; i++) kf_idx[fill[ob[i].kf]++] = i;
  LbaKf* kf = S.kf;
  for (int k = 0; k < H.n_kf; k++) {
    memcpy(kf[k].p, kfs[k].nav.p, 24);
    kf[k].qw = kfs[k].nav.q[0], kf[k].qx = kfs[k].nav.q[1];
    kf[k].qy = kfs[k].nav.q[2], kf[k].qz = kfs[k].nav.q[3];
    kf[k].col = -1, kf[k].fixed = kfs[k].fixed ? 1 : 0;
    memcpy(kf[k].v, kfs[k].nav.v, 24), memcpy(kf[k].dbg, kfs[k].nav.dbg, 24), memcpy(kf[k].dba, kfs[k].nav.dba, 24);
    memcpy(kf[k].bg, kfs[k].nav.bg, 24), memcpy(kf[k].ba, kfs[k].nav.ba, 24);
  }
  if (H.VP) {  // inertial edges (Optimizer.cc:226-311)
    LbaImu* im = staged(S.imu);
    for (int t = 0; t < H.n_imu; t++) {
      const vieo_lba_imu_edge& e = c.h_imu[w][t];
      LbaImu& d = im[t];
      d.i = e.kf_i, d.j = e.kf_j, d.M = e.imu;
      const bool bfixedkf = kfs[e.kf_i].fixed != 0;
      d.has_imu = e.imu.dt != 0, d.robust = c.gba ? c.gba->robust != 0 : (bfixedkf || H.VP->rec_init);
      memset(d.InfoI, 0, sizeof(d.InfoI));
      if (d.has_imu) {
        if (!inverse_n(e.imu.Sigma, d.InfoI, 9)) {
          set_error("visual-inertial local BA: singular pre-integration covariance");
          return VIEO_E_INVALID;
        }
        if (bfixedkf)
          for (int q = 0; q < 81; q++) d.InfoI[q] *= 1e-2;
      }
      double deltatij = e.imu.dt ? e.imu.dt : e.dt_kf;
      const float EPS_MIN_DT = 1e-6f;
      if (deltatij <= EPS_MIN_DT) deltatij = 15;  // Optimizer.cc:271-275
      d.infoBg = H.VP->inv_sigma_bg2 / deltatij * (bfixedkf ? 1e-2 : 1.0);
      d.infoBa = H.VP->inv_sigma_ba2 / deltatij * (bfixedkf ? 1e-2 : 1.0);
      memset(d.InfoE, 0, sizeof(d.InfoE)), memset(d.measE, 0, sizeof(d.measE));
      if (!fill_enc_edge(d, e.enc, bfixedkf, enc_robust)) {
        set_error("visual-inertial local BA: singular encoder covariance");
        return VIEO_E_INVALID;
      }
    }
    fill_chain(S, H);
    if (c.h_close[w])
      memcpy(staged(S.close), c.h_close[w], H.n_mp);
    else
      memset(staged(S.close), 0, H.n_mp);
  } else if (H.ENC) {  // encoder edges only: no inertial residual, no bias random walk
    LbaImu* im = staged(S.imu);
    for (int t = 0; t < H.n_imu; t++) {
      const vieo_lba_enc_edge& e = H.ENC->edges[t];
      LbaImu& d = im[t];
      memset(&d, 0, sizeof(d));
      d.i = e.kf_i, d.j = e.kf_j;
      if (!fill_enc_edge(d, e.enc, kfs[e.kf_i].fixed != 0, enc_robust)) {
        set_error("local BA: singular encoder covariance");
        return VIEO_E_INVALID;
      }
    }
    fill_chain(S, H);
    memset(staged(S.close), 0, H.n_mp);
  }
  for (int i = 0; i < H.n_mp * 3; i++) S.X[i] = (double)c.h_points[w][i];
  memset(S.erase, 0, H.n_obs);
  S.scl[0] = S.scl[1] = 1.0;  // pvScale->setEstimate(1.) (Optimizer.cc:845)
  if (H.cls == 3) {
    int* d = staged(S.sch_ptr);  // the first of plan_lists(): the block's start
    LbaDev unused;
    for (auto& l : plan_lists(H.plan, &unused))
      if (!l.first->empty()) memcpy(d, l.first->data(), l.first->size() * 4), d += l.first->size();
  }
  return VIEO_OK;
}

// Staging: the inputs of every window into the pinned copy `hs` of the arena.  Windows are independent and the work is
// memory copies, so a large batch is split over a few host threads (6.6 ms on one thread for the 103 windows of a
// bench step).
static int lba_stage(const LbaCall& c, const std::vector<WinHost>& win, std::vector<LbaDev>& devs, LbaLayout& L, uint8_t* hs) {
  std::vector<int> live;
  for (int w = 0; w < c.W; w++)
    if (!win[w].skip) live.push_back(w), arena_bind(L.win[w], win[w], devs[w], R_IN, R_ZERO, hs);
  auto fill = [&](int w) { return fill_window(c, w, win[w], devs[w]); };
  const int hw = (int)std::thread::hardware_concurrency();
  const int nt = std::max(1, std::min(std::min(8, hw > 0 ? hw : 1), (int)live.size() / 8));
  std::vector<int> rcs(live.size(), VIEO_OK);
  if (nt <= 1) {
    for (size_t i = 0; i < live.size(); i++)
      if ((rcs[i] = fill(live[i])) != VIEO_OK) return rcs[i];
    return VIEO_OK;
  }
  std::vector<std::thread> th;
  for (int t = 0; t < nt; t++)
    th.emplace_back([&, t] {
      for (size_t i = t; i < live.size(); i += nt) rcs[i] = fill(live[i]);
    });
  for (auto& x : th) x.join();
  for (size_t i = 0; i < live.size(); i++)
    if (rcs[i] != VIEO_OK) return fill(live[i]);  // again on this thread: the error text is thread-local
  return VIEO_OK;
}

// The device side of the descriptors: the arena (reserved here), the pointers into it, a sharded run's slices of the
// reduction buffer.
static int lba_describe(const LbaCall& c, const std::vector<WinHost>& win, std::vector<LbaDev>& devs, LbaLayout& L, LbaGrids& G) {
  const int W = c.W;
  int rc;
  if (G.cls_max[3] > 0) {
    // the tile-sparse solve's limit is device memory: its pool, Schur tiles and lists are part of the arena
    size_t fr = 0, tot = 0;
    int cur = 0;
    (void)hipGetDevice(&cur);
    VIEO_HIP_CHECK(hipMemGetInfo(&fr, &tot));
    const size_t have = fr + (g_arena.p && g_arena.dev == cur ? g_arena.cap : 0);
    if (L.arena > have) {
      size_t plan_b = 0;
      for (int w = 0; w < W; w++)
        if (win[w].cls == 3) plan_b += win[w].plan.bytes(devs[w].ksplit);
      set_error("bundle adjustment: the tile-sparse solve needs %zu bytes of device memory (%zu of them the tile pool, "
                "Schur tiles and plan), %zu are free",
                L.arena, plan_b, have);
      return VIEO_E_CAPACITY;
    }
  }
  if ((rc = g_arena.ensure(L.arena)) != VIEO_OK) return rc;
  for (int w = 0; w < W; w++)
    if (win[w].cls == 3) {
      const GbaSparsePlan& P = win[w].plan;
      std::lock_guard<std::mutex> g(g_lba_kt_mutex);
      g_lba_sparse_stats[0] = (long long)P.n_tiles(), g_lba_sparse_stats[1] = (long long)P.nt * (P.nt + 1) / 2;
      g_lba_sparse_stats[2] = (long long)P.n_sch_tiles(), g_lba_sparse_stats[3] = (long long)P.vrb * P.vcb - (long long)P.vrb * (P.vrb - 1) / 2;
      g_lba_sparse_stats[4] = (long long)P.bytes(devs[w].ksplit), g_lba_sparse_stats[5] = (long long)L.arena;
    }
  if ((rc = g_small.ensure((size_t)W * (sizeof(LbaDev) + sizeof(WinCtl) + sizeof(WinOut) + sizeof(int)))) != VIEO_OK) return rc;
  if ((rc = g_small_h.ensure((size_t)W * (sizeof(WinCtl) + sizeof(WinOut) + 32))) != VIEO_OK) return rc;
  for (int w = 0; w < W; w++)
    if (!win[w].skip) arena_bind(L.win[w], win[w], devs[w], R_IN, R_N, g_arena.as<uint8_t>());
  if (const LbaShard* sh = c.sh) {
    for (int w = 0; w < W; w++) {
      if (win[w].skip) continue;
      devs[w].red = sh->d_buf + G.shard_sys;
      G.shard_sys += shard_sys_doubles(devs[w].nf_cap, c.sco());
    }
    if (G.shard_sys + 4 * (size_t)W > sh->cap) {
      set_error("sharded local BA: reduction buffer too small (%zu doubles needed)", G.shard_sys + 4 * (size_t)W);
      return VIEO_E_CAPACITY;
    }
    for (int w = 0; w < W; w++) devs[w].red_sc = sh->d_buf + G.shard_sys + 4 * (size_t)w;
  }
  return VIEO_OK;
}

struct LbaBufs {  // the small per-window records of a call, on the device and pinned on the host
  LbaDev* dD;
  WinCtl* dC;
  WinOut* dO;
  int* dWins;  // the windows grouped by solver class: [class 0 | class 1 | class 2 | class 3] (LbaGrids::cls_order)
  WinCtl* ctl;
  WinOut* out;
  double* h_sc;  // reduced scalars of a sharded run
};

static LbaBufs lba_bufs(int W) {
  LbaBufs B;
  B.dD = g_small.as<LbaDev>();
  B.dC = (WinCtl*)(B.dD + W), B.dO = (WinOut*)(B.dC + W), B.dWins = (int*)(B.dO + W);
  B.ctl = (WinCtl*)g_small_h.p, B.out = (WinOut*)(B.ctl + W), B.h_sc = (double*)(B.out + W);
  return B;
}

// Everything a call sends ahead of its rounds: the staged arena, the descriptors, the class table.
static int lba_enqueue(const LbaCall& c, const LbaLayout& L, const std::vector<LbaDev>& devs, const LbaGrids& G,
                       const LbaBufs& B, const uint8_t* hs, hipStream_t st) {
  const int W = c.W;
  uint8_t* base = g_arena.as<uint8_t>();
  VIEO_HIP_CHECK(hipMemcpyAsync(base, hs, L.res_end, hipMemcpyHostToDevice, st));
  VIEO_HIP_CHECK(hipMemsetAsync(base + L.res_end, 0, L.zero_end - L.res_end, st));
  VIEO_HIP_CHECK(hipMemcpyAsync(B.dD, devs.data(), (size_t)W * sizeof(LbaDev), hipMemcpyHostToDevice, st));
  VIEO_HIP_CHECK(hipMemsetAsync(B.dO, 0, (size_t)W * sizeof(WinOut), st));
  if (!G.cls_order.empty())
    VIEO_HIP_CHECK(hipMemcpyAsync(B.dWins, G.cls_order.data(), G.cls_order.size() * sizeof(int), hipMemcpyHostToDevice, st));
  if (G.cls_max[1] > 0)
    VIEO_HIP_CHECK(hipFuncSetAttribute((const void*)k_lba_ldltg<kLdGThreads>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)ldg_lds_bytes(G.nbg)));
  if (G.cls_max[0] > 0)
    VIEO_HIP_CHECK(hipFuncSetAttribute((const void*)k_lba_ldlt16<kLd16Threads>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)ld16_lds_bytes(G.nb16)));
  return VIEO_OK;
}

// The tiled LDL^T over many workgroups, dense (class 2) or over the stored tiles of the fill pattern (class 3): nt
// panels -- panel_grid(k) the rows under panel k's diagonal tile, syrk_grid(k) its update targets -- then the back
// substitution of n unknowns.
template <bool TILES, class PanelGrid, class SyrkGrid>
static void launch_big_ldlt(LbaKTimer& KT, int kc, const LbaBufs& B, int W, hipStream_t st, int nt, int n,
                            PanelGrid panel_grid, SyrkGrid syrk_grid) {
  LbaDev* dD = B.dD;
  WinCtl* dC = B.dC;
  WinOut* dO = B.dO;
  for (int k = 0; k < nt; k++) {
    KT.launch(kc, [&] { hipLaunchKernelGGL(k_big_panel<TILES>, dim3(panel_grid(k), W), dim3(256), 0, st, dD, dC, k); });
    if (syrk_grid(k) > 0)
      KT.launch(kc, [&] { hipLaunchKernelGGL(k_big_syrk<TILES>, dim3(syrk_grid(k), W), dim3(256), 0, st, dD, dC, k); });
  }
  for (int sb = 0; sb < (n + kNB - 1) / kNB; sb++)
    KT.launch(kc, [&] { hipLaunchKernelGGL(k_big_back_step<TILES>, dim3(1 + (n + 255) / 256, W), dim3(256), 0, st, dD, dC, sb); });
  KT.launch(kc, [&] { hipLaunchKernelGGL(k_big_finish<TILES>, dim3(W), dim3(256), 0, st, dD, dC, dO); });
}

// The launch schedule of one round.  any: the windows' control words or-ed together; cls_trial[c]: a window of solver
// class c takes a trial this round.
static int launch_round(const LbaCall& c, const LbaGrids& G, const LbaBufs& B, LbaKTimer& KT, int any,
                        const bool* cls_trial, hipStream_t st) {
  const LbaShard* sh = c.sh;
  const int W = c.W, sco = c.sco();
  const int ge = G.ge, gq = G.gq, gr = G.gr, max_chunks = G.max_chunks, max_imu = G.max_imu, max_nf = G.max_nf;
  const int* cls_max = G.cls_max;
  const int* cls_first = G.cls_first;
  LbaDev* dD = B.dD;
  WinCtl* dC = B.dC;
  WinOut* dO = B.dO;
  int* dWins = B.dWins;
  int rc;
  VIEO_HIP_CHECK(hipMemcpyAsync(dC, B.ctl, (size_t)W * sizeof(WinCtl), hipMemcpyHostToDevice, st));
  if (any & LBA_RESTORE) KT.launch(KC_OTHER, [&] { hipLaunchKernelGGL(k_lba_restore, dim3(gr, W), dim3(256), 0, st, dD, dC); });
  if (any & (LBA_CLASS0 | LBA_CLASS1)) KT.launch(KC_OTHER, [&] { hipLaunchKernelGGL(k_lba_classify, dim3(ge, W), dim3(256), 0, st, dD, dC); });
  if (any & LBA_PRELEVEL)
    for (int ph = 0; ph < 3; ph++) KT.launch(KC_OTHER, [&] { hipLaunchKernelGGL(k_lba_prelevel, dim3(ge, W), dim3(256), 0, st, dD, dC, ph); });
  if (any & LBA_BEGIN) {
    KT.launch(KC_BEGIN, [&] { hipLaunchKernelGGL(k_lba_zero, dim3(64, W), dim3(256), 0, st, dD, dC); });
    KT.launch(KC_BEGIN, [&] { hipLaunchKernelGGL(k_lba_begin, dim3(W), dim3(1024), 0, st, dD, dC, dO); });
    if (c.gba) KT.launch(KC_BEGIN, [&] { hipLaunchKernelGGL(k_lba_occ, dim3(std::max(1, (G.occ_max + 255) / 256), W), dim3(256), 0, st, dD, dC); });
    KT.launch(KC_ERROR, [&] { hipLaunchKernelGGL(k_lba_error, dim3(ge, W), dim3(256), 0, st, dD, dC, 0); });
  }
  if (any & LBA_BUILD) {
    auto build2 = [&](auto mc, auto sc) {  // point half, key-frame half
      constexpr bool MC = decltype(mc)::value, SC = decltype(sc)::value;
      if (G.fused_build) {  // one launch for both halves
        KT.launch(KC_BUILD, [&] { hipLaunchKernelGGL((k_lba_build<MC, SC, 2>), dim3(gq + max_chunks + max_imu, W), dim3(256), 0, st, dD, dC, max_chunks, gq); });
        if (W > 4) KT.launch(KC_BUILD, [&] { hipLaunchKernelGGL(k_lba_build_fold, dim3(std::max(1, max_nf), W), dim3(64), 0, st, dD, dC); });
        return;
      }
      KT.launch(KC_BUILD, [&] { hipLaunchKernelGGL((k_lba_build<MC, SC, 0>), dim3(gq, W), dim3(256), 0, st, dD, dC, 0, 0); });
      KT.launch(KC_BUILD, [&] { hipLaunchKernelGGL((k_lba_build<MC, SC, 1>), dim3(max_chunks, W), dim3(256), 0, st, dD, dC, max_chunks, 0); });
      if (W > 4) KT.launch(KC_BUILD, [&] { hipLaunchKernelGGL(k_lba_build_fold, dim3(std::max(1, max_nf), W), dim3(64), 0, st, dD, dC); });
    };
    if (sco) {
      if (G.any_multicam)
        build2(std::true_type(), std::true_type());
      else
        build2(std::false_type(), std::true_type());
      KT.launch(KC_BUILD, [&] { hipLaunchKernelGGL(k_lba_scale_fold, dim3(W), dim3(256), 0, st, dD, dC); });
    } else if (G.any_multicam)
      build2(std::true_type(), std::false_type());
    else
      build2(std::false_type(), std::false_type());
    if (!G.fused_build && max_imu > 0) KT.launch(KC_GENERIC, [&] { hipLaunchKernelGGL(k_lba_generic, dim3(max_imu, W), dim3(64), 0, st, dD, dC, 0); });
  }
  if (any & LBA_BEGIN) KT.launch(KC_BEGIN, [&] { hipLaunchKernelGGL(k_lba_lambda, dim3(W), dim3(256), 0, st, dD, dC, dO); });
  if (!(any & LBA_TRIAL)) return VIEO_OK;
  const bool sparse_trial = cls_max[3] > 0 && cls_trial[3];
  if (cls_max[0] > 0 || cls_max[1] > 0 || cls_max[2] > 0) {
    KT.launch(KC_SCHUR, [&] { hipLaunchKernelGGL(k_lba_schur<false>, dim3(std::max(1, G.schur), W), dim3(256), 0, st, dD, dC, dO); });
    if (G.schur_off > 0)
      KT.launch(KC_SCHUR, [&] { hipLaunchKernelGGL(k_lba_schur<true>, dim3(G.schur_off, W), dim3(256), 0, st, dD, dC, dO); });
  }
  if (sparse_trial) {  // the planned tiles only
    KT.launch(KC_SCHUR, [&] { hipLaunchKernelGGL((k_lba_schur<false, true>), dim3(std::max(1, G.schur_t), W), dim3(256), 0, st, dD, dC, dO); });
    if (G.schur_t_off > 0)
      KT.launch(KC_SCHUR, [&] { hipLaunchKernelGGL((k_lba_schur<true, true>), dim3(G.schur_t_off, W), dim3(256), 0, st, dD, dC, dO); });
  }
  if (sh) {  // the one exchange step of the path: sum the reduced visual system over the ranks
    KT.launch(KC_OTHER, [&] { hipLaunchKernelGGL(k_lba_pack, dim3((unsigned)((shard_sys_doubles(max_nf, sco) + 255) / 256), W), dim3(256), 0, st,
                       dD, dC); });
    if ((rc = shard_exchange(sh, sh->d_buf, G.shard_sys, st)) != VIEO_OK) return rc;
  }
  for (int cl = 1; cl < 3; cl++) {  // (class 0: k_lba_ldlt16 forms its system itself)
    const int nw = cls_first[cl + 1] - cls_first[cl];
    if (nw <= 0 || !cls_trial[cl]) continue;
    const unsigned gx = (unsigned)(((size_t)cls_max[cl] * cls_max[cl] + 255) / 256);
    KT.launch(KC_ASSEMBLE, [&] { hipLaunchKernelGGL(k_lba_assemble, dim3(gx, nw), dim3(256), 0, st, dD, dC, dO, dWins + cls_first[cl]); });
  }
  if (cls_max[2] > 0 && cls_trial[2]) {
    const int n = cls_max[2], nbm = (n + 1 + kNB - 1) / kNB * kNB, ntm = nbm / kNB;
    KT.launch(KC_LDLT, [&] { hipLaunchKernelGGL(k_big_init, dim3((unsigned)(((size_t)nbm * nbm + 255) / 256), W), dim3(256), 0, st, dD, dC); });
    launch_big_ldlt<false>(
        KT, KC_LDLT, B, W, st, ntm, n, [&](int k) { return 1 + (nbm - (k + 1) * kNB + 255) / 256; },
        [&](int k) { return (ntm - k - 1) * (ntm - k) / 2; });
  }
  if (sparse_trial) {  // the tile-sparse LDL^T: assembly into the pool, then the planned tiles' panels
    const int nw = cls_first[4] - cls_first[3];
    const unsigned ga = (unsigned)std::min<size_t>(16384, std::max<size_t>(1, (G.sp_elems + 255) / 256));
    KT.launch(KC_ASSEMBLE, [&] { hipLaunchKernelGGL(k_lba_assemble_tiles, dim3(ga, nw), dim3(256), 0, st, dD, dC, dO, dWins + cls_first[3]); });
    launch_big_ldlt<true>(
        KT, KC_LDLT_SPARSE, B, W, st, G.sp_nt, cls_max[3], [&](int k) { return G.sp_panel_grid[k]; },
        [&](int k) { return G.sp_syrk_grid[k]; });
  }
  if (cls_max[0] > 0 && cls_trial[0])
    KT.launch(KC_LDLT, [&] { hipLaunchKernelGGL(k_lba_ldlt16<kLd16Threads>, dim3(W), dim3(kLd16Threads), ld16_lds_bytes(G.nb16), st, dD, dC, dO, G.nb16); });
  if (cls_max[1] > 0 && cls_trial[1])
    KT.launch(KC_LDLT, [&] { hipLaunchKernelGGL(k_lba_ldltg<kLdGThreads>, dim3(W), dim3(kLdGThreads), ldg_lds_bytes(G.nbg), st, dD, dC, dO, G.nbg); });
  if (G.fused_tail)
    KT.launch(KC_UPDATE, [&] { hipLaunchKernelGGL(k_lba_tail, dim3(gq + max_imu, W), dim3(256), 0, st, dD, dC, dO, gq); });
  else {
    KT.launch(KC_UPDATE, [&] { hipLaunchKernelGGL(k_lba_update_points, dim3(gq, W), dim3(256), 0, st, dD, dC, dO); });
    KT.launch(KC_ERROR, [&] { hipLaunchKernelGGL(k_lba_error, dim3(ge, W), dim3(256), 0, st, dD, dC, 1); });
    if (max_imu > 0) KT.launch(KC_GENERIC, [&] { hipLaunchKernelGGL(k_lba_generic, dim3(max_imu, W), dim3(64), 0, st, dD, dC, 1); });
    KT.launch(KC_OTHER, [&] { hipLaunchKernelGGL(k_lba_reduce, dim3(W), dim3(256), 0, st, dD, dC, dO); });
  }
  if (sh) {  // chi2 and the landmark part of the gain-ratio scale
    if ((rc = shard_exchange(sh, sh->d_buf + G.shard_sys, 4 * (size_t)W, st)) != VIEO_OK) return rc;
    VIEO_HIP_CHECK(hipMemcpyAsync(B.h_sc, sh->d_buf + G.shard_sys, 32 * (size_t)W, hipMemcpyDeviceToHost, st));
  }
  VIEO_HIP_CHECK(hipMemcpyAsync(B.out, dO, (size_t)W * sizeof(WinOut), hipMemcpyDeviceToHost, st));
  return VIEO_OK;
}

// Results of the windows that took part, from the staging copy `hs` of the arena's result region.
static void lba_write_back(const LbaCall& c, std::vector<WinHost>& win, const uint8_t* hs) {
  const bool vio = c.vio();
  for (int w = 0; w < c.W; w++) {
    WinHost& H = win[w];
    if (H.skip) continue;
    vieo_lba_result* R = H.lm.R;
    if (vio) {  // float err / err_end and the divergence guard (Optimizer.cc:531-533,655-666)
      const float err = (float)R->chi2_initial, err_end = (float)H.lm.lastTrialChi;
      R->chi2_initial = err, R->chi2_final = err_end;
      if ((2 * err < err_end || std::isnan(err) || std::isnan(err_end)) && !H.VP->large && !c.gba) {
        R->status = VIEO_LBA_DIVERGED;
        continue;  // returns without write-back: outputs stay equal to the inputs
      }
    }
    if (H.n_obs > 0) memcpy(c.h_erase[w], hs + H.o_erase, H.n_obs);
    for (int i = 0; i < H.n_obs; i++) R->n_erase += c.h_erase[w][i];
    const LbaKf* o = (const LbaKf*)(hs + H.o_kf);
    const double* X = (const double*)(hs + H.o_X);
    vieo_navstate* navs = c.h_navs_out[w];
    for (int k = 0; k < H.n_kf; k++) {
      if (c.h_kfs[w][k].fixed) continue;
      memcpy(navs[k].p, o[k].p, 24);
      navs[k].q[0] = o[k].qw, navs[k].q[1] = o[k].qx, navs[k].q[2] = o[k].qy, navs[k].q[3] = o[k].qz;
      if (vio) {  // ns_recov: v of the V vertex, dbg / dba of the Bias vertex (Optimizer.cc:716-733)
        memcpy(navs[k].v, o[k].v, 24);
        memcpy(navs[k].dbg, o[k].dbg, 24), memcpy(navs[k].dba, o[k].dba, 24);
      }
    }
    float* pts = c.h_points_out[w];
    if (c.sco()) {  // SetWorldPos(scale * vPoint->estimate().cast<float>()) (Optimizer.cc:1321): a float product
      const double scale = *(const double*)(hs + H.o_scl);
      const float sf = (float)scale;
      for (int i = 0; i < H.n_mp * 3; i++) pts[i] = sf * (float)X[i];
      if (c.gba->scale_out) *c.gba->scale_out = scale;
    } else
      for (int i = 0; i < H.n_mp * 3; i++) pts[i] = (float)X[i];  // SetWorldPos(cast<float>)
  }
}

static int lba_run(const LbaCall& c) {
  const LbaShard* sh = c.sh;
  const int W = c.W;
  if (c.gba && c.gba->scale_out) *c.gba->scale_out = 1.0;
  bool shard_stop = false;  // a sharded run's collective view of the stop flag (latched)
  int rc = lba_check_and_agree(c, &shard_stop);
  if (rc != VIEO_OK) return rc;
  ShardStagingGuard staging_guard{sh};  // from here to the second agreement every early return reports to the other ranks
  hipStream_t st;
  if ((rc = lba_stream(&st)) != VIEO_OK) return rc;
  // VIEO_LBA_TIMING=1: host phases of a call on stderr (staging, rounds, results)
  static const bool host_timing = getenv("VIEO_LBA_TIMING") != nullptr;
  const auto t_enter = std::chrono::steady_clock::now();
  auto ms_since = [](std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
  };
  std::vector<WinHost> win(W);
  if (!lba_open_windows(c, sh ? shard_stop : c.stop_raised(), win)) {
    staging_guard.done = true;  // (key frames and stop state are replicated: the ranks of a sharded run all leave here together)
    return VIEO_OK;
  }
  std::vector<LbaDev> devs(W);
  LbaLayout L;
  LbaGrids G;
  lba_layout(c, win, devs, L, G);
  if ((rc = g_stage.ensure(L.res_end)) != VIEO_OK) return rc;
  uint8_t* hs = (uint8_t*)g_stage.p;
  const double ms_layout = ms_since(t_enter);
  if ((rc = lba_stage(c, win, devs, L, hs)) != VIEO_OK) return rc;
  const double ms_filled = ms_since(t_enter);
  if ((rc = lba_describe(c, win, devs, L, G)) != VIEO_OK) return rc;
  const LbaBufs B = lba_bufs(W);
  const double ms_described = ms_since(t_enter);
  if ((rc = lba_enqueue(c, L, devs, G, B, hs, st)) != VIEO_OK) return rc;
  if (sh) {  // second agreement: every rank staged its windows (ShardStagingGuard reports the ones that did not)
    VIEO_HIP_CHECK(hipStreamSynchronize(st));
    double sum = 1.0;
    staging_guard.done = true;
    const int xrc = shard_agree(sh, true, &sum);
    if (xrc != VIEO_OK) return xrc;
    if (sum != 0.0) {
      set_error("sharded local BA: another rank failed while staging its windows, all ranks return");
      return VIEO_E_INVALID;
    }
  }
  // ---- lock-step rounds: plan the round, launch it, wait, digest the trials
  const double ms_staged = ms_since(t_enter);
  const auto t_rounds = std::chrono::steady_clock::now();
  int n_rounds = 0;
  double ms_wait = 0;
  static thread_local LbaKTimer KT;
  KT.begin(st);
  const LmMode mode = c.lm_mode();
  for (;;) {
    n_rounds++;
    const bool stop_now = sh ? shard_stop : c.stop_raised();
    const int stop_req = sh && c.stop_raised() ? 1 : 0;  // (sharded: travels as ctl.pad -> the trial's fourth scalar)
    int any = 0;
    bool cls_trial[4] = {false, false, false, false};  // which solve kernels have a window this round
    for (int w = 0; w < W; w++) {
      B.ctl[w] = lm_plan_round(win[w].lm, mode, stop_now, stop_req);
      any |= B.ctl[w].flags;
      if ((B.ctl[w].flags & LBA_TRIAL) && !win[w].skip) cls_trial[win[w].cls] = true;
    }
    if (!any) break;
    if ((rc = launch_round(c, G, B, KT, any, cls_trial, st)) != VIEO_OK) return rc;
    VIEO_HIP_CHECK(hipGetLastError());
    {
      const auto t_w = std::chrono::steady_clock::now();
      VIEO_HIP_CHECK(hipStreamSynchronize(st));
      ms_wait += ms_since(t_w);
    }
    if (KT.on) {
      // the windows this round's k_lba_schur launch worked on: dense count 2 np (np + 1) 3 n_mp of the visual part of
      // a window's Schur complement
      double fl = 0;
      for (int w = 0; w < W; w++)
        if ((B.ctl[w].flags & LBA_TRIAL) && !win[w].skip)
          fl += 2.0 * (6 * devs[w].nf_cap) * (6 * devs[w].nf_cap + 1) * 3.0 * devs[w].n_mp;
      KT.fold(fl);
    }
    if (sh)  // the ranks' stop requests of this round (the same count in every window that ran a trial)
      for (int w = 0; w < W; w++)
        if (lm_shard_stop_requested(B.ctl[w].flags, B.h_sc + 4 * w)) shard_stop = true;
    for (int w = 0; w < W; w++)
      lm_digest_trial(win[w].lm, mode, B.ctl[w].flags, B.out[w], sh ? B.h_sc + 4 * w : nullptr,
                      sh ? shard_stop : c.stop_raised());
  }
  // ---- results: one copy for all windows
  const double ms_rounds = ms_since(t_rounds);
  const auto t_res = std::chrono::steady_clock::now();
  VIEO_HIP_CHECK(hipMemcpyAsync(hs + L.res_begin, g_arena.as<uint8_t>() + L.res_begin, L.res_end - L.res_begin,
                                hipMemcpyDeviceToHost, st));
  VIEO_HIP_CHECK(hipStreamSynchronize(st));
  if (host_timing)
    fprintf(stderr, "lba_run: %d windows, staging %.3f ms, %d rounds %.3f ms (of which waiting for the stream %.3f), "
                    "results copy %.3f ms; staging: layout %.3f, windows filled %.3f, descriptors %.3f, enqueued %.3f\n", W, ms_staged,
            n_rounds, ms_rounds, ms_wait, ms_since(t_res), ms_layout, ms_filled, ms_described, ms_staged);
  lba_write_back(c, win, hs);
  return VIEO_OK;
}

}  // namespace vieo

using namespace vieo;

// a full BA has no erase flags to return: one window, with a throw-away array in their place
static int gba_run(LbaCall& c, const GbaMode& g, int n_obs) {
  std::vector<uint8_t> erase((size_t)std::max(n_obs, 1));
  uint8_t* er = erase.data();
  c.gba = &g, c.W = 1, c.h_erase = &er;
  return lba_run(c);
}

extern "C" {

int vieo_lba_set_stream_priority(int priority) {
  if (priority < -1 || priority > 1) return VIEO_E_INVALID;
  if (priority != g_lba_priority && g_lba_stream) {  // the next call creates the stream again
    (void)hipStreamSynchronize(g_lba_stream);
    (void)hipStreamDestroy(g_lba_stream);
    g_lba_stream = nullptr;
  }
  g_lba_priority = priority;
  return VIEO_OK;
}

int vieo_local_bundle_adjustment_batch_enc(int n_windows, const vieo_lba_params* const* params,
                                           const vieo_lba_keyframe* const* h_kfs, const int* n_kf,
                                           const float* const* h_points, const int* n_mp,
                                           const vieo_lba_obs* const* h_obs, const int* n_obs,
                                           const vieo_lba_enc* const* encs, volatile const int* stop,
                                           vieo_navstate* const* h_navs_out, float* const* h_points_out,
                                           uint8_t* const* h_erase, vieo_lba_result* h_results) {
  LbaCall c;
  c.W = n_windows, c.params = params, c.encs = encs;
  c.h_kfs = h_kfs, c.n_kf = n_kf, c.h_points = h_points, c.n_mp = n_mp, c.h_obs = h_obs, c.n_obs = n_obs;
  c.stop = stop;
  c.h_navs_out = h_navs_out, c.h_points_out = h_points_out, c.h_erase = h_erase, c.h_results = h_results;
  return lba_run(c);
}

int vieo_local_bundle_adjustment_batch(int n_windows, const vieo_lba_params* const* params,
                                       const vieo_lba_keyframe* const* h_kfs, const int* n_kf,
                                       const float* const* h_points, const int* n_mp,
                                       const vieo_lba_obs* const* h_obs, const int* n_obs,
                                       volatile const int* stop, vieo_navstate* const* h_navs_out,
                                       float* const* h_points_out, uint8_t* const* h_erase,
                                       vieo_lba_result* h_results) {
  return vieo_local_bundle_adjustment_batch_enc(n_windows, params, h_kfs, n_kf, h_points, n_mp, h_obs, n_obs, nullptr, stop,
                                                h_navs_out, h_points_out, h_erase, h_results);
}

int vieo_local_bundle_adjustment(const vieo_lba_params* P, const vieo_lba_keyframe* h_kfs, int n_kf,
                                 const float* h_points, int n_mp, const vieo_lba_obs* h_obs, int n_obs,
                                 volatile const int* stop, vieo_navstate* h_navs_out,
                                 float* h_points_out, uint8_t* h_erase, vieo_lba_result* R) {
  return vieo_local_bundle_adjustment_enc(P, h_kfs, n_kf, h_points, n_mp, h_obs, n_obs, nullptr, stop, h_navs_out, h_points_out,
                                          h_erase, R);
}

int vieo_local_bundle_adjustment_enc(const vieo_lba_params* P, const vieo_lba_keyframe* h_kfs, int n_kf,
                                     const float* h_points, int n_mp, const vieo_lba_obs* h_obs, int n_obs,
                                     const vieo_lba_enc* enc, volatile const int* stop, vieo_navstate* h_navs_out,
                                     float* h_points_out, uint8_t* h_erase, vieo_lba_result* R) {
  if (!P || !h_kfs || n_kf <= 0 || !h_points || n_mp <= 0 || !h_obs || n_obs <= 0 || !h_navs_out ||
      !h_points_out || !h_erase || !R)
    return VIEO_E_INVALID;
  return vieo_local_bundle_adjustment_batch_enc(1, &P, &h_kfs, &n_kf, &h_points, &n_mp, &h_obs, &n_obs, &enc, stop,
                                                &h_navs_out, &h_points_out, &h_erase, R);
}

int vieo_bundle_adjustment_enc(const vieo_lba_params* params, int n_iterations, int robust,
                               const vieo_lba_keyframe* h_kfs, int n_kf, const float* h_points, int n_mp,
                               const vieo_lba_obs* h_obs, int n_obs, const vieo_lba_enc* enc,
                               volatile const int* stop, vieo_navstate* h_navs_out, float* h_points_out,
                               vieo_lba_result* h_result) {
  if (!params || n_iterations < 0 || !h_result || n_obs < 0) return VIEO_E_INVALID;
  const GbaMode g = {n_iterations, robust};
  LbaCall c;
  c.params = &params, c.encs = &enc;
  c.h_kfs = &h_kfs, c.n_kf = &n_kf, c.h_points = &h_points, c.n_mp = &n_mp, c.h_obs = &h_obs, c.n_obs = &n_obs;
  c.stop = stop;
  c.h_navs_out = &h_navs_out, c.h_points_out = &h_points_out, c.h_results = h_result;
  return gba_run(c, g, n_obs);
}

int vieo_bundle_adjustment(const vieo_lba_params* params, int n_iterations, int robust,
                           const vieo_lba_keyframe* h_kfs, int n_kf, const float* h_points, int n_mp,
                           const vieo_lba_obs* h_obs, int n_obs, volatile const int* stop, vieo_navstate* h_navs_out,
                           float* h_points_out, vieo_lba_result* h_result) {
  return vieo_bundle_adjustment_enc(params, n_iterations, robust, h_kfs, n_kf, h_points, n_mp, h_obs, n_obs, nullptr, stop,
                                    h_navs_out, h_points_out, h_result);
}

int vieo_local_bundle_adjustment_vio_batch(int n_windows, const vieo_lba_vio_params* const* params,
                                           const vieo_lba_keyframe* const* h_kfs, const int* n_kf,
                                           const float* const* h_points, const uint8_t* const* h_close,
                                           const int* n_mp, const vieo_lba_obs* const* h_obs, const int* n_obs,
                                           const vieo_lba_imu_edge* const* h_imu, const int* n_imu,
                                           volatile const int* stop, vieo_navstate* const* h_navs_out,
                                           float* const* h_points_out, uint8_t* const* h_erase,
                                           vieo_lba_result* h_results) {
  if (!params) return VIEO_E_INVALID;
  LbaCall c;
  c.W = n_windows, c.vparams = params;
  c.h_kfs = h_kfs, c.n_kf = n_kf, c.h_points = h_points, c.h_close = h_close, c.n_mp = n_mp;
  c.h_obs = h_obs, c.n_obs = n_obs, c.h_imu = h_imu, c.n_imu = n_imu;
  c.stop = stop;
  c.h_navs_out = h_navs_out, c.h_points_out = h_points_out, c.h_erase = h_erase, c.h_results = h_results;
  return lba_run(c);
}

int vieo_local_bundle_adjustment_vio(const vieo_lba_vio_params* P, const vieo_lba_keyframe* h_kfs, int n_kf,
                                     const float* h_points, const uint8_t* h_close, int n_mp,
                                     const vieo_lba_obs* h_obs, int n_obs, const vieo_lba_imu_edge* h_imu,
                                     int n_imu, volatile const int* stop, vieo_navstate* h_navs_out,
                                     float* h_points_out, uint8_t* h_erase, vieo_lba_result* R) {
  if (!P || !h_kfs || n_kf <= 0 || !h_points || !h_close || n_mp <= 0 || !h_obs || n_obs <= 0 || n_imu < 0 ||
      (n_imu > 0 && !h_imu) || !h_navs_out || !h_points_out || !h_erase || !R)
    return VIEO_E_INVALID;
  return vieo_local_bundle_adjustment_vio_batch(1, &P, &h_kfs, &n_kf, &h_points, &h_close, &n_mp, &h_obs, &n_obs,
                                                &h_imu, &n_imu, stop, &h_navs_out, &h_points_out, &h_erase, R);
}

size_t vieo_lba_sharded_buffer_doubles(int n_windows, const int* n_free_kf) {
  size_t n = 0;
  for (int w = 0; w < n_windows; w++) n += shard_sys_doubles(n_free_kf ? n_free_kf[w] : 0, 1) + 4;  // (room for the scale vertex)
  return n;
}

int vieo_local_bundle_adjustment_vio_sharded_stop(int n_windows, const vieo_lba_vio_params* const* params,
                                                  const vieo_lba_keyframe* const* h_kfs, const int* n_kf,
                                                  const float* const* h_points, const uint8_t* const* h_close,
                                                  const int* n_mp, const vieo_lba_obs* const* h_obs, const int* n_obs,
                                                  const vieo_lba_imu_edge* const* h_imu, const int* n_imu,
                                                  double* d_reduce_buf, size_t reduce_cap_doubles,
                                                  vieo_allreduce_sum_f64_fn allreduce, void* ctx, volatile const int* stop,
                                                  vieo_navstate* const* h_navs_out, float* const* h_points_out,
                                                  uint8_t* const* h_erase, vieo_lba_result* h_results) {
  if (!params) return VIEO_E_INVALID;
  const LbaShard sh{allreduce, ctx, d_reduce_buf, reduce_cap_doubles};
  LbaCall c;
  c.sh = &sh;
  c.W = n_windows, c.vparams = params;
  c.h_kfs = h_kfs, c.n_kf = n_kf, c.h_points = h_points, c.h_close = h_close, c.n_mp = n_mp;
  c.h_obs = h_obs, c.n_obs = n_obs, c.h_imu = h_imu, c.n_imu = n_imu;
  c.stop = stop;
  c.h_navs_out = h_navs_out, c.h_points_out = h_points_out, c.h_erase = h_erase, c.h_results = h_results;
  return lba_run(c);
}

int vieo_local_bundle_adjustment_vio_sharded(int n_windows, const vieo_lba_vio_params* const* params,
                                             const vieo_lba_keyframe* const* h_kfs, const int* n_kf,
                                             const float* const* h_points, const uint8_t* const* h_close,
                                             const int* n_mp, const vieo_lba_obs* const* h_obs, const int* n_obs,
                                             const vieo_lba_imu_edge* const* h_imu, const int* n_imu,
                                             double* d_reduce_buf, size_t reduce_cap_doubles,
                                             vieo_allreduce_sum_f64_fn allreduce, void* ctx,
                                             vieo_navstate* const* h_navs_out, float* const* h_points_out,
                                             uint8_t* const* h_erase, vieo_lba_result* h_results) {
  return vieo_local_bundle_adjustment_vio_sharded_stop(n_windows, params, h_kfs, n_kf, h_points, h_close, n_mp, h_obs, n_obs, h_imu,
                                                       n_imu, d_reduce_buf, reduce_cap_doubles, allreduce, ctx, nullptr, h_navs_out,
                                                       h_points_out, h_erase, h_results);
}

// the visual-inertial full BAs: sh == nullptr, or one rank of a landmark-sharded run
static int gba_vio_run(const LbaShard* sh, const vieo_lba_vio_params* params, int n_iterations, int robust, int scale_opt,
                       const vieo_lba_keyframe* h_kfs, int n_kf, const float* h_points, int n_mp,
                       const vieo_lba_obs* h_obs, int n_obs, const vieo_lba_imu_edge* h_imu, int n_imu,
                       volatile const int* stop, vieo_navstate* h_navs_out, float* h_points_out,
                       vieo_lba_result* h_result, double* h_scale_out) {
  if (!params || n_iterations < 0 || !h_result || n_obs < 0) return VIEO_E_INVALID;
  GbaMode g = {n_iterations, robust};
  g.scale_opt = scale_opt != 0, g.scale_out = h_scale_out;
  const uint8_t* no_close = nullptr;
  LbaCall c;
  c.sh = sh;
  c.vparams = &params;
  c.h_kfs = &h_kfs, c.n_kf = &n_kf, c.h_points = &h_points, c.h_close = &no_close, c.n_mp = &n_mp;
  c.h_obs = &h_obs, c.n_obs = &n_obs, c.h_imu = &h_imu, c.n_imu = &n_imu;
  c.stop = stop;
  c.h_navs_out = &h_navs_out, c.h_points_out = &h_points_out, c.h_results = h_result;
  return gba_run(c, g, n_obs);
}

int vieo_global_bundle_adjustment_vio_sharded_scale(const vieo_lba_vio_params* params, int n_iterations, int robust,
                                                    int scale_opt, const vieo_lba_keyframe* h_kfs, int n_kf,
                                                    const float* h_points, int n_mp, const vieo_lba_obs* h_obs, int n_obs,
                                                    const vieo_lba_imu_edge* h_imu, int n_imu, double* d_reduce_buf,
                                                    size_t reduce_cap_doubles, vieo_allreduce_sum_f64_fn allreduce,
                                                    void* ctx, vieo_navstate* h_navs_out, float* h_points_out,
                                                    vieo_lba_result* h_result, double* h_scale_out) {
  const LbaShard sh{allreduce, ctx, d_reduce_buf, reduce_cap_doubles};
  return gba_vio_run(&sh, params, n_iterations, robust, scale_opt, h_kfs, n_kf, h_points, n_mp, h_obs, n_obs, h_imu, n_imu,
                     nullptr, h_navs_out, h_points_out, h_result, h_scale_out);
}

int vieo_global_bundle_adjustment_vio_sharded(const vieo_lba_vio_params* params, int n_iterations, int robust,
                                              const vieo_lba_keyframe* h_kfs, int n_kf, const float* h_points,
                                              int n_mp, const vieo_lba_obs* h_obs, int n_obs,
                                              const vieo_lba_imu_edge* h_imu, int n_imu, double* d_reduce_buf,
                                              size_t reduce_cap_doubles, vieo_allreduce_sum_f64_fn allreduce,
                                              void* ctx, vieo_navstate* h_navs_out, float* h_points_out,
                                              vieo_lba_result* h_result) {
  return vieo_global_bundle_adjustment_vio_sharded_scale(params, n_iterations, robust, 0, h_kfs, n_kf, h_points, n_mp,
                                                         h_obs, n_obs, h_imu, n_imu, d_reduce_buf, reduce_cap_doubles,
                                                         allreduce, ctx, h_navs_out, h_points_out, h_result, nullptr);
}

int vieo_global_bundle_adjustment_vio_scale(const vieo_lba_vio_params* params, int n_iterations, int robust, int scale_opt,
                                            const vieo_lba_keyframe* h_kfs, int n_kf, const float* h_points, int n_mp,
                                            const vieo_lba_obs* h_obs, int n_obs, const vieo_lba_imu_edge* h_imu,
                                            int n_imu, volatile const int* stop, vieo_navstate* h_navs_out,
                                            float* h_points_out, vieo_lba_result* h_result, double* h_scale_out) {
  return gba_vio_run(nullptr, params, n_iterations, robust, scale_opt, h_kfs, n_kf, h_points, n_mp, h_obs, n_obs, h_imu, n_imu,
                     stop, h_navs_out, h_points_out, h_result, h_scale_out);
}

int vieo_global_bundle_adjustment_vio(const vieo_lba_vio_params* params, int n_iterations, int robust,
                                      const vieo_lba_keyframe* h_kfs, int n_kf, const float* h_points, int n_mp,
                                      const vieo_lba_obs* h_obs, int n_obs, const vieo_lba_imu_edge* h_imu, int n_imu,
                                      volatile const int* stop, vieo_navstate* h_navs_out, float* h_points_out,
                                      vieo_lba_result* h_result) {
  return vieo_global_bundle_adjustment_vio_scale(params, n_iterations, robust, 0, h_kfs, n_kf, h_points, n_mp, h_obs, n_obs,
                                                 h_imu, n_imu, stop, h_navs_out, h_points_out, h_result, nullptr);
}

// Kernel-class timing of the bundle-adjustment engine (bench.py's roofline over the whole path).
void vieo_lba_enable_timing(int on) {
  std::lock_guard<std::mutex> g(vieo::g_lba_kt_mutex);
  vieo::g_lba_ktiming.store(on == 2 ? 2 : (on ? 1 : 0));
  for (int i = 0; i < vieo::KC_N; i++) vieo::g_lba_kt_ms[i] = 0, vieo::g_lba_kt_launches[i] = 0;
  vieo::g_lba_kt_schur_flops = 0;
}
int vieo_lba_kernel_classes(void) { return vieo::KC_N; }
const char* vieo_lba_kernel_class_name(int i) { return i >= 0 && i < vieo::KC_N ? vieo::kLbaKClassName[i] : ""; }
void vieo_lba_kernel_times(double* ms, long long* launches, double* schur_flops) {
  std::lock_guard<std::mutex> g(vieo::g_lba_kt_mutex);
  for (int i = 0; i < vieo::KC_N; i++) ms[i] = vieo::g_lba_kt_ms[i], launches[i] = vieo::g_lba_kt_launches[i];
  *schur_flops = vieo::g_lba_kt_schur_flops;
}
void vieo_lba_sparse_stats(long long* out) {
  std::lock_guard<std::mutex> g(vieo::g_lba_kt_mutex);
  for (int i = 0; i < 6; i++) out[i] = vieo::g_lba_sparse_stats[i];
}
}  // extern "C"
