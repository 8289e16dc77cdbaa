// lba_device.h -- the records of the bundle-adjustment engine (lba.hip) and the per-edge algebra its stages share:
// LbaKf / LbaImu / LbaDev, the accessors (win_scale .. write_kf_xf), the visual edge's residual and Jacobians
// (EdgeReprojectPR[Stereo], reference src/Odom/g2otypes.h:321-547), win_lambda, landmark_dinv.  No kernel in here.
// LbaDev is one window's descriptor, an element of the array every kernel takes as `devs`: plan_window / arena_bind
// (lba.hip) fill it on the host -- counts, thresholds, cameras, pointers into the call's arena -- and k_lba_begin writes
// np, n_free, npv, n_chunks on the device.  Every kernel loads its fields by offset, so the field order is part of
// the kernels' code.  The stage headers (lba_inertial_device.h, lba_state_device.h, lba_linearize_device.h,
// lba_schur_device.h, lba_solve_device.h) say which fields their kernels read and write.
// xf, the transform table, is written where the states change -- k_lba_prelevel(0) / k_lba_begin, lba_apply_step,
// k_lba_restore, all through write_kf_xf -- and read by every visual edge.
//
// Full BA with bScaleOpt (System::FinalGBA, src/System.cc:24-33; Optimizer.cc:842-851,1131-1137,1190-1196,1256-1335):
// the VertexScale (g2otypes.h:292-311) is one more 1-dim column at the END of the pose system and the visual edges are
// EdgeReprojectPRS / PRSStereo (g2otypes.h:321-541, MODE_OPT_VAR == 1): Xw = s Xh, J_s = (Jproj Rcw) Xh,
// J_Xh = s (Jproj Rcw).  The scale sees every point, so it is one more (dense) row of BB -- row 6 x free key frames --
// and the Schur GEMM, the pack / all-reduce and the solves take it like any other row; its own blocks (H_ss, b_s,
// H_ps) are summed in fixed order by k_lba_build / k_lba_scale_fold and gathered by lba_assemble_entry_at.
#pragma once
#include "ba_device.h"
#include "lba_policy.h"

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

}  // namespace vieo
