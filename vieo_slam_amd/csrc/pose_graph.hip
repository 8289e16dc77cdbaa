// pose_graph.hip -- Optimizer::OptimizeEssentialGraph (Optimizer.cc:2309-2687) on the device: one Sim3 vertex per key
// frame, one EdgeSim3 per edge, g2o's Levenberg-Marquardt (host policy: lba_policy.h) with g2o's numeric Jacobians, a
// tile-sparse LDL^T of the pose block system, then the SE3 poses and the map-point correction.
//
// Unknowns: pd = 6 (fix_scale: the scale column of every Jacobian is exactly zero, so row / column 6 of H would hold
// lambda alone and x[6] = 0) or 7 per free vertex, in key-frame order, no reordering.  A vertex is free when it is
// valid, not the fixed one and has an edge (g2o's active set).  H is kept as 64 x 64 FP64 tiles of the lower triangle
// inside the row envelope: tile row r holds tile columns first[r] .. r, first[r] the leftmost tile an edge of the row
// reaches.  A right-looking LDL^T fills nothing outside that envelope, so a loop edge fills the tile rows of the late
// key frames only.  The right-hand side travels as one more tile row (row 0 of it): after the factorisation it holds
// D^-1 L^-1 b, and one back substitution is left.  Every sum has one owner thread and a fixed order: no floating-point
// atomics anywhere, and the result does not depend on the launch geometry.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "common.h"
#include "lba_policy.h"
#include "pose_graph_plan.h"
#include "sim3_device.h"

namespace vieo {
namespace {

constexpr int TS = kPgTile;   // tile side
constexpr int TT = TS * TS;   // doubles per tile
constexpr int LIN_LANES = 32; // lanes of an edge in k_pg_linearize: 28 perturbed evaluations + the plain one

struct EdgeBlk {  // the quadratic form of one edge (BaseBinaryEdge::constructQuadraticForm)
  double Hii[49], Hij[49], Hjj[49], bi[7], bj[7];
};

using AsmItem = PgAsmItem;  // one 7 x 7 block of H: pose_graph_plan.h

__device__ inline double info_w(const double* info, int e, int k) { return k < 3 ? info[2 * e] : k < 6 ? info[2 * e + 1] : 1.0; }

__device__ inline size_t tile_at(const int* tile_off, const int* tfirst, int r, int c) {
  return (size_t)(tile_off[r] + c - tfirst[r]) * TT;
}

// measurement of every edge from the two tables (Optimizer.cc:2400-2417, :2477-2611)
__global__ void k_pg_measure(int n_edges, const Sim3* Scw, const Sim3* Scw_prior, const int* ei, const int* ej, const int* kind,
                             Sim3* meas) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_edges) return;
  const Sim3* T = kind[e] == VIEO_PG_EDGE_LOOP ? Scw : Scw_prior;
  meas[e] = s3_mul(T[ej[e]], s3_inverse(T[ei[e]]));
}

// e = log(C Si Sj^-1) and both Jacobians by g2o's central differences (delta = 1e-9) through the vertex's oplus
// (S <- exp(u) S, u[6] = 0 under fix_scale): lane 2 (7 v + d) + s of an edge's 32 evaluates vertex v, dimension d, sign s;
// lane 28 the plain error.  Then the edge's quadratic form.  blockDim.x / 32 edges per block.
__global__ void k_pg_linearize(int n_edges, const Sim3* est, const Sim3* meas, const int* ei, const int* ej, const double* info,
                               int fix_scale, double* err, double* chi, EdgeBlk* blk, double* Ji_out, double* Jj_out) {
  __shared__ double sh_e[8][29][7];
  __shared__ double sh_J[8][2][49];
  const int le = threadIdx.x / LIN_LANES, lane = threadIdx.x % LIN_LANES;
  const int e = blockIdx.x * (blockDim.x / LIN_LANES) + le;
  const bool live = e < n_edges;
  if (live && lane < 29) {
    Sim3 Si = est[ei[e]], Sj = est[ej[e]];
    if (lane < 28) {
      const int v = lane / 14, d = (lane % 14) >> 1;
      double u[7];
      for (int k = 0; k < 7; k++) u[k] = k == d ? ((lane & 1) ? -1e-9 : 1e-9) : 0.0;
      if (fix_scale) u[6] = 0;
      const Sim3 P = s3_exp(u);
      if (v == 0)
        Si = s3_mul(P, Si);
      else
        Sj = s3_mul(P, Sj);
    }
    double r[7];
    s3_edge_error(meas[e], Si, Sj, r);
    for (int k = 0; k < 7; k++) sh_e[le][lane][k] = r[k];
  }
  __syncthreads();
  if (live) {
    const double scalar = 1.0 / (2 * 1e-9);
    for (int t = lane; t < 98; t += LIN_LANES) {
      const int v = t / 49, row = (t % 49) / 7, col = t % 7;
      const int lp = v * 14 + col * 2;
      sh_J[le][v][row * 7 + col] = scalar * (sh_e[le][lp][row] - sh_e[le][lp + 1][row]);
    }
  }
  __syncthreads();
  if (!live) return;
  const double* E = sh_e[le][28];
  const double* A = sh_J[le][0];
  const double* B = sh_J[le][1];
  if (lane < 7 && err) err[7 * (size_t)e + lane] = E[lane];
  if (lane == 0 && chi) {
    double c = 0;
    for (int k = 0; k < 7; k++) c += E[k] * (info_w(info, e, k) * E[k]);
    chi[e] = c;
  }
  if (Ji_out)
    for (int t = lane; t < 49; t += LIN_LANES) Ji_out[49 * (size_t)e + t] = A[t], Jj_out[49 * (size_t)e + t] = B[t];
  if (!blk) return;
  EdgeBlk& O = blk[e];
  for (int t = lane; t < 161; t += LIN_LANES) {
    if (t < 147) {
      const int which = t / 49, a = (t % 49) / 7, b = t % 7;
      const double* L = which == 2 ? B : A;
      const double* R = which == 0 ? A : B;
      double s = 0;
      for (int k = 0; k < 7; k++) s += (L[k * 7 + a] * info_w(info, e, k)) * R[k * 7 + b];
      (which == 0 ? O.Hii : which == 1 ? O.Hij : O.Hjj)[a * 7 + b] = s;
    } else {
      const int which = (t - 147) / 7, a = (t - 147) % 7;
      const double* L = which ? B : A;
      double s = 0;
      for (int k = 0; k < 7; k++) s += L[k * 7 + a] * (-(info_w(info, e, k) * E[k]));
      (which ? O.bj : O.bi)[a] = s;
    }
  }
}

// chi2 of every edge at the current estimates (computeActiveErrors after a trial's update)
__global__ void k_pg_errors(int n_edges, const Sim3* est, const Sim3* meas, const int* ei, const int* ej, const double* info,
                            double* chi) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_edges) return;
  double r[7];
  s3_edge_error(meas[e], est[ei[e]], est[ej[e]], r);
  double c = 0;
  for (int k = 0; k < 7; k++) c += r[k] * (info_w(info, e, k) * r[k]);
  chi[e] = c;
}

// identity on the diagonal of the last tile's unused rows
__global__ void k_pg_pad(int n, int T, const int* tile_off, const int* tfirst, double* H) {
  const int r = n + blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= T * TS) return;
  H[tile_at(tile_off, tfirst, T - 1, T - 1) + (size_t)(r % TS) * TS + r % TS] = 1.0;
}

// J^T Omega J and -J^T Omega e into the tiles: 64 threads per item, each entry the sum over its edges in edge order
__global__ void k_pg_assemble(int n_items, const AsmItem* items, const int* refs, const EdgeBlk* blk, int pd, int T,
                              const int* tile_off, const int* tfirst, double* H, double* bvec) {
  const int it = (blockIdx.x * blockDim.x + threadIdx.x) / 64, t = threadIdx.x % 64;
  if (it >= n_items || t >= 56) return;
  const AsmItem I = items[it];
  if (t < 49) {
    const int a = t / 7, b = t % 7;
    if (a >= pd || b >= pd) return;
    double s = 0;
    for (int k = I.begin; k < I.end; k++) {
      const EdgeBlk& B = blk[refs[k] >> 1];
      const int f = refs[k] & 1;
      s += I.diag ? (f ? B.Hjj : B.Hii)[a * 7 + b] : (f ? B.Hij[b * 7 + a] : B.Hij[a * 7 + b]);
    }
    const int row = I.rbase + a, col = I.cbase + b;
    if (row / TS >= col / TS) H[tile_at(tile_off, tfirst, row / TS, col / TS) + (size_t)(row % TS) * TS + col % TS] = s;
  } else if (I.diag) {
    const int a = t - 49;
    if (a >= pd) return;
    double s = 0;
    for (int k = I.begin; k < I.end; k++) {
      const EdgeBlk& B = blk[refs[k] >> 1];
      s += ((refs[k] & 1) ? B.bj : B.bi)[a];
    }
    const int row = I.rbase + a;
    bvec[row] = s;
    H[tile_at(tile_off, tfirst, T, row / TS) + row % TS] = s;  // row 0 of the right-hand side's tile row
  }
}

// LDL^T of diagonal tile k (+ lambda on its diagonal): unit L below the diagonal, D on it.  One block of 256.
__global__ void __launch_bounds__(256) k_pg_ldl_diag(double* W, const int* tile_off, const int* tfirst, int k, double lambda, int* ok) {
  __shared__ double a[TS][TS + 1];
  double* tile = W + tile_at(tile_off, tfirst, k, k);
  for (int idx = threadIdx.x; idx < TT; idx += 256) {
    const int i = idx / TS, j = idx % TS;
    if (j <= i) a[i][j] = tile[idx] + (i == j ? lambda : 0.0);
  }
  __syncthreads();
  for (int j = 0; j < TS; j++) {
    double d = a[j][j];
    const bool bad = !(d > 0.0) || !(d < 1.7e308);
    if (bad) d = 1.0;  // the trial has failed (ok = 0); keep the arithmetic finite
    __syncthreads();
    if (threadIdx.x == 0 && bad) *ok = 0, a[j][j] = 1.0;
    if ((int)threadIdx.x > j && threadIdx.x < TS) a[threadIdx.x][j] = a[threadIdx.x][j] / d;
    __syncthreads();
    for (int idx = threadIdx.x; idx < TT; idx += 256) {
      const int i = idx / TS, c = idx % TS;
      if (c > j && c <= i) a[i][c] -= (a[i][j] * d) * a[c][j];
    }
    __syncthreads();
  }
  for (int idx = threadIdx.x; idx < TT; idx += 256) {
    const int i = idx / TS, j = idx % TS;
    if (j <= i) tile[idx] = a[i][j];
  }
}

// panel of tile column k: L(r, k) = A(r, k) L(k, k)^-T D^-1, one block of 64 per row tile, one thread per row
__global__ void __launch_bounds__(64) k_pg_ldl_panel(double* W, const int* tile_off, const int* tfirst, int k, const int* rows) {
  __shared__ double Lp[TS * (TS + 1) / 2];
  __shared__ double yT[TS][TS];
  const int r = rows[blockIdx.x], i = threadIdx.x;
  const double* Lkk = W + tile_at(tile_off, tfirst, k, k);
  double* X = W + tile_at(tile_off, tfirst, r, k);
  for (int idx = i; idx < TT; idx += TS) {
    const int a = idx / TS, b = idx % TS;
    if (b <= a) Lp[a * (a + 1) / 2 + b] = Lkk[idx];
    yT[b][a] = X[idx];
  }
  __syncthreads();
  for (int j = 0; j < TS; j++) {
    double acc = yT[j][i];
    const double* Lj = Lp + j * (j + 1) / 2;
    for (int p = 0; p < j; p++) acc -= yT[p][i] * Lj[p];
    yT[j][i] = acc;
  }
  __syncthreads();
  for (int idx = i; idx < TT; idx += TS) {
    const int a = idx / TS, b = idx % TS;
    X[idx] = yT[b][a] / Lp[b * (b + 1) / 2 + b];
  }
}

// trailing update of tile column k: A(r, c) -= L(r, k) D L(c, k)^T for every pair r >= c of its row list
__global__ void __launch_bounds__(256) k_pg_ldl_update(double* W, const int* tile_off, const int* tfirst, int k, const int* rows) {
  const int r = rows[blockIdx.x], c = rows[blockIdx.y];
  if (r < c) return;
  __shared__ double As[32][TS], Bs[32][TS];
  const double* Lr = W + tile_at(tile_off, tfirst, r, k);
  const double* Lc = W + tile_at(tile_off, tfirst, c, k);
  const double* Dk = W + tile_at(tile_off, tfirst, k, k);
  double* O = W + tile_at(tile_off, tfirst, r, c);
  const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;
  double acc[4][4] = {};
  for (int half = 0; half < 2; half++) {
    for (int idx = threadIdx.x; idx < 32 * TS; idx += 256) {
      const int p = idx % 32, i = idx / 32, g = half * 32 + p;
      As[p][i] = Lr[i * TS + g];
      Bs[p][i] = Lc[i * TS + g] * Dk[g * TS + g];
    }
    __syncthreads();
    for (int p = 0; p < 32; p++)
      for (int ii = 0; ii < 4; ii++)
        for (int jj = 0; jj < 4; jj++) acc[ii][jj] += As[p][ty * 4 + ii] * Bs[p][tx * 4 + jj];
    __syncthreads();
  }
  for (int ii = 0; ii < 4; ii++)
    for (int jj = 0; jj < 4; jj++) O[(ty * 4 + ii) * TS + tx * 4 + jj] -= acc[ii][jj];
}

// x = L^-T z, z = row 0 of the right-hand side's tile row after the factorisation.  One block of 64.
__global__ void __launch_bounds__(64) k_pg_ldl_back(const double* W, const int* tile_off, const int* tfirst, int T,
                                                    const int* list_off, const int* rows, double* x) {
  __shared__ double xs[TS];
  const int j = threadIdx.x;
  for (int k = T - 1; k >= 0; k--) {
    double acc = W[tile_at(tile_off, tfirst, T, k) + j];
    for (int q = list_off[k]; q < list_off[k + 1] - 1; q++) {  // (the list's last entry is the right-hand side's row)
      const int r = rows[q];
      const double* L = W + tile_at(tile_off, tfirst, r, k);
      const double* xr = x + (size_t)r * TS;
      for (int i = 0; i < TS; i++) acc -= L[i * TS + j] * xr[i];
    }
    xs[j] = acc;
    __syncthreads();
    const double* Lkk = W + tile_at(tile_off, tfirst, k, k);
    for (int i = TS - 1; i > 0; i--) {
      const double xi = xs[i];
      if (j < i) xs[j] -= Lkk[i * TS + j] * xi;
      __syncthreads();
    }
    x[(size_t)k * TS + j] = xs[j];
    __syncthreads();
  }
}

// oplus per free vertex, with the backup a rejected trial restores; its term of g2o's computeScale
__global__ void k_pg_update(int n_free, const int* free_kf, int pd, const double* x, const double* bvec, double lambda,
                            Sim3* est, Sim3* backup, double* scale_v) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_free) return;
  const int kf = free_kf[f];
  double u[7], s = 0;
  for (int d = 0; d < 7; d++) {
    u[d] = d < pd ? x[(size_t)f * pd + d] : 0.0;
    if (d < pd) s += u[d] * (lambda * u[d] + bvec[(size_t)f * pd + d]);
  }
  const Sim3 S = est[kf];
  backup[kf] = S;
  est[kf] = s3_mul(s3_exp(u), S);
  scale_v[f] = s;
}

// chi2 = sum of chi[n_a], scale = sum of sv[n_b], each in one fixed order (256 strided partial sums, then a tree)
__global__ void __launch_bounds__(256) k_pg_reduce(const double* chi, int n_a, const double* sv, int n_b, const int* ok, double* rec,
                                                   int trial) {
  __shared__ double sa[256], sb[256];
  double a = 0, b = 0;
  for (int i = threadIdx.x; i < n_a; i += 256) a += chi[i];
  for (int i = threadIdx.x; i < n_b; i += 256) b += sv[i];
  sa[threadIdx.x] = a, sb[threadIdx.x] = b;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sa[threadIdx.x] += sa[threadIdx.x + w], sb[threadIdx.x] += sb[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (trial)
      rec[1] = sa[0], rec[2] = sb[0], rec[3] = (double)*ok;
    else
      rec[0] = sa[0];
  }
}

// Tcw = R | t / s of every valid key frame (Optimizer.cc:2636-2644) and the map-point correction (:2670-2679)
__global__ void k_pg_finish(int n_kf, const uint8_t* valid, const Sim3* est, const Sim3* Scw, double* Tcw, int n_mp, const float* Pw,
                            const int* ref_kf, float* Pw_out, double* Pw_out_d) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n_kf) {
    double* o = Tcw + 12 * (size_t)t;
    if (valid[t]) {
      double R[9];
      s3_quat_to_mat(est[t].q, R);
      const double inv = 1. / est[t].s;
      for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) o[4 * i + j] = R[3 * i + j];
        o[4 * i + 3] = est[t].t[i] * inv;
      }
    } else
      for (int i = 0; i < 12; i++) o[i] = 0;
  }
  if (t < n_mp) {
    const int r = ref_kf[t];
    const double p[3] = {(double)Pw[3 * (size_t)t], (double)Pw[3 * (size_t)t + 1], (double)Pw[3 * (size_t)t + 2]};
    double o[3] = {p[0], p[1], p[2]};
    if (r >= 0) {
      double a[3];
      s3_map(Scw[r], p, a);
      s3_map(s3_inverse(est[r]), a, o);
    }
    for (int i = 0; i < 3; i++) {
      Pw_out[3 * (size_t)t + i] = r >= 0 ? (float)o[i] : Pw[3 * (size_t)t + i];
      if (Pw_out_d) Pw_out_d[3 * (size_t)t + i] = o[i];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
struct Arena {  // offsets into one device allocation
  size_t used = 0;
  size_t take(size_t bytes) {
    const size_t off = used;
    used += (bytes + 255) & ~(size_t)255;
    return off;
  }
};

int validate(const vieo_pose_graph* g, bool with_points) {
  if (!g || g->n_kf <= 0 || g->n_edges < 0 || g->n_mp < 0 || !g->valid || !g->Scw || !g->Scw_prior) {
    set_error("pose graph: null pointer or negative count");
    return VIEO_E_INVALID;
  }
  if (g->n_edges && (!g->edge_i || !g->edge_j || !g->edge_kind || !g->edge_info)) {
    set_error("pose graph: null edge arrays");
    return VIEO_E_INVALID;
  }
  if (g->fixed_kf < 0 || g->fixed_kf >= g->n_kf || !g->valid[g->fixed_kf] || g->n_iterations < 0) {
    set_error("pose graph: fixed_kf %d is not a valid key frame of 0..%d (or n_iterations < 0)", g->fixed_kf, g->n_kf - 1);
    return VIEO_E_INVALID;
  }
  for (int e = 0; e < g->n_edges; e++) {
    const int i = g->edge_i[e], j = g->edge_j[e], k = g->edge_kind[e];
    if (i < 0 || j < 0 || i >= g->n_kf || j >= g->n_kf || i == j || !g->valid[i] || !g->valid[j] ||
        (k != VIEO_PG_EDGE_LOOP && k != VIEO_PG_EDGE_PRIOR)) {
      set_error("pose graph: edge %d (%d, %d, kind %d) names a key frame out of range, an invalid one or itself", e, i, j, k);
      return VIEO_E_INVALID;
    }
  }
  if (with_points && g->n_mp) {
    if (!g->Pw || !g->ref_kf) {
      set_error("pose graph: null map-point arrays");
      return VIEO_E_INVALID;
    }
    for (int p = 0; p < g->n_mp; p++)
      if (g->ref_kf[p] >= g->n_kf || (g->ref_kf[p] >= 0 && !g->valid[g->ref_kf[p]])) {
        set_error("pose graph: map point %d refers to key frame %d", p, g->ref_kf[p]);
        return VIEO_E_INVALID;
      }
  }
  return VIEO_OK;
}

bool alt_geometry() {
  const char* s = getenv("VIEO_PG_GEOMETRY");
  return s && !strcmp(s, "alt");
}

template <class T>
size_t vbytes(const std::vector<T>& v) { return v.size() * sizeof(T); }

// the factor and its lists must fit into device memory next to the per-edge and per-vertex tables
int check_capacity(const PgPlan& P, int ne, int nk, int nmp, size_t held, unsigned long long* bytes_needed) {
  const unsigned long long need = (unsigned long long)P.tiles * TT * 8 * 2 + (unsigned long long)ne * (sizeof(EdgeBlk) + 200) +
                                  (unsigned long long)nk * 200 + (unsigned long long)nmp * 48 + ((unsigned long long)64 << 20);
  size_t fr = 0, tot = 0;
  VIEO_HIP_CHECK(hipMemGetInfo(&fr, &tot));
  if (P.n_ll > 0x7fffffff / 2 || P.tiles > 0x3fffffff || need + need / 2 > fr + held) {
    *bytes_needed = need;
    set_error("pose graph: %d unknowns need %llu bytes of device memory for the factor, %zu are free", P.n, need, fr);
    return VIEO_E_CAPACITY;
  }
  return VIEO_OK;
}

// The device side of one linear system (H + lambda I) x = b: the plan's lists, H in tiles, the copy the factorisation
// works in, b and x.  Both callers -- the optimisation and the test tap vieo_pose_graph_solve -- assemble and solve
// through it, so they launch the same kernels with the same geometry.
struct PgSystem {
  const PgPlan* P = nullptr;
  size_t o_items = 0, o_refs = 0, o_tfirst = 0, o_toff = 0, o_loff = 0, o_rows = 0, o_x = 0, o_b = 0, o_H = 0, o_W = 0;
  size_t tile_bytes = 0;
  uint8_t* d = nullptr;  // the arena, once it is allocated

  void take(Arena& A, const PgPlan& plan, bool structured) {
    P = &plan;
    o_items = A.take(vbytes(plan.items)), o_refs = A.take(vbytes(plan.refs)), o_tfirst = A.take(vbytes(plan.tfirst));
    o_toff = A.take(vbytes(plan.tile_off)), o_loff = A.take(vbytes(plan.list_off)), o_rows = A.take(vbytes(plan.rows));
    const size_t n_pad = (size_t)(plan.T + 1) * TS;
    o_x = A.take(8 * n_pad), o_b = A.take(8 * n_pad);
    tile_bytes = structured ? (size_t)plan.tile_off[plan.T + 1] * TT * 8 : 0;
    o_H = A.take(tile_bytes), o_W = A.take(tile_bytes);
  }
  int* tfirst() const { return (int*)(d + o_tfirst); }
  int* toff() const { return (int*)(d + o_toff); }
  int* rows() const { return (int*)(d + o_rows); }
  double* H() const { return (double*)(d + o_H); }
  double* W() const { return (double*)(d + o_W); }
  double* x() const { return (double*)(d + o_x); }
  double* b() const { return (double*)(d + o_b); }

  int upload(uint8_t* arena, hipStream_t st) {
    d = arena;
#define PG_UP(off, v) \
  if (vbytes(v)) VIEO_HIP_CHECK(hipMemcpyAsync(d + (off), (v).data(), vbytes(v), hipMemcpyHostToDevice, st))
    PG_UP(o_items, P->items);
    PG_UP(o_refs, P->refs);
    PG_UP(o_tfirst, P->tfirst);
    PG_UP(o_toff, P->tile_off);
    PG_UP(o_loff, P->list_off);
    PG_UP(o_rows, P->rows);
#undef PG_UP
    return VIEO_OK;
  }
  // H and b from the edges' quadratic forms
  int assemble(const EdgeBlk* blk, int bs, hipStream_t st) {
    const int n = P->n, T = P->T;
    VIEO_HIP_CHECK(hipMemsetAsync(H(), 0, tile_bytes, st));
    if (T * TS > n) k_pg_pad<<<1, TS, 0, st>>>(n, T, toff(), tfirst(), H());
    const int nit = (int)P->items.size();
    k_pg_assemble<<<(nit * 64 + bs - 1) / bs, bs, 0, st>>>(nit, (AsmItem*)(d + o_items), (int*)(d + o_refs), blk, P->pd, T, toff(),
                                                           tfirst(), H(), b());
    return VIEO_OK;
  }
  // (H + lambda I) x = b; *ok stays non-zero unless a pivot is not positive
  int solve(double lambda, int* ok, hipStream_t st) {
    const int T = P->T;
    const std::vector<int>& list_off = P->list_off;
    VIEO_HIP_CHECK(hipMemcpyAsync(W(), H(), tile_bytes, hipMemcpyDeviceToDevice, st));
    VIEO_HIP_CHECK(hipMemsetAsync(ok, 0xff, 4, st));  // any non-zero value: no bad pivot so far
    for (int k = 0; k < T; k++) {
      const int m = list_off[k + 1] - list_off[k];
      k_pg_ldl_diag<<<1, 256, 0, st>>>(W(), toff(), tfirst(), k, lambda, ok);
      k_pg_ldl_panel<<<m, TS, 0, st>>>(W(), toff(), tfirst(), k, rows() + list_off[k]);
      if (m > 1) k_pg_ldl_update<<<dim3(m, m - 1), 256, 0, st>>>(W(), toff(), tfirst(), k, rows() + list_off[k]);
    }
    k_pg_ldl_back<<<1, TS, 0, st>>>(W(), toff(), tfirst(), T, (int*)(d + o_loff), rows(), x());
    return VIEO_OK;
  }
};

}  // namespace
}  // namespace vieo

using namespace vieo;

extern "C" int vieo_pose_graph_linearize(const vieo_pose_graph* g, double* e, double* Ji, double* Jj) {
  int rc;
  if ((rc = validate(g, false)) != VIEO_OK) return rc;
  if (!e || !Ji || !Jj) {
    set_error("vieo_pose_graph_linearize: null output");
    return VIEO_E_INVALID;
  }
  if ((rc = require_device()) != VIEO_OK) return rc;
  if (g->n_edges == 0) return VIEO_OK;
  static thread_local DevBuf buf;
  const int ne = g->n_edges, nk = g->n_kf;
  Arena A;
  const size_t o_scw = A.take(sizeof(Sim3) * nk), o_pri = A.take(sizeof(Sim3) * nk), o_meas = A.take(sizeof(Sim3) * ne);
  const size_t o_ei = A.take(4 * (size_t)ne), o_ej = A.take(4 * (size_t)ne), o_kind = A.take(4 * (size_t)ne);
  const size_t o_info = A.take(16 * (size_t)ne), o_e = A.take(56 * (size_t)ne), o_ji = A.take(392 * (size_t)ne),
               o_jj = A.take(392 * (size_t)ne);
  if ((rc = buf.ensure(A.used)) != VIEO_OK) return rc;
  uint8_t* d = buf.as<uint8_t>();
  hipStream_t st = 0;
  VIEO_HIP_CHECK(hipMemcpyAsync(d + o_scw, g->Scw, sizeof(Sim3) * nk, hipMemcpyHostToDevice, st));
  VIEO_HIP_CHECK(hipMemcpyAsync(d + o_pri, g->Scw_prior, sizeof(Sim3) * nk, hipMemcpyHostToDevice, st));
  VIEO_HIP_CHECK(hipMemcpyAsync(d + o_ei, g->edge_i, 4 * (size_t)ne, hipMemcpyHostToDevice, st));
  VIEO_HIP_CHECK(hipMemcpyAsync(d + o_ej, g->edge_j, 4 * (size_t)ne, hipMemcpyHostToDevice, st));
  VIEO_HIP_CHECK(hipMemcpyAsync(d + o_kind, g->edge_kind, 4 * (size_t)ne, hipMemcpyHostToDevice, st));
  VIEO_HIP_CHECK(hipMemcpyAsync(d + o_info, g->edge_info, 16 * (size_t)ne, hipMemcpyHostToDevice, st));
  const int bs = alt_geometry() ? 128 : 256, epb = bs / LIN_LANES;
  k_pg_measure<<<(ne + bs - 1) / bs, bs, 0, st>>>(ne, (Sim3*)(d + o_scw), (Sim3*)(d + o_pri), (int*)(d + o_ei), (int*)(d + o_ej),
                                                  (int*)(d + o_kind), (Sim3*)(d + o_meas));
  k_pg_linearize<<<(ne + epb - 1) / epb, bs, 0, st>>>(ne, (Sim3*)(d + o_scw), (Sim3*)(d + o_meas), (int*)(d + o_ei),
                                                      (int*)(d + o_ej), (double*)(d + o_info), g->fix_scale != 0,
                                                      (double*)(d + o_e), nullptr, nullptr, (double*)(d + o_ji),
                                                      (double*)(d + o_jj));
  VIEO_HIP_CHECK(hipGetLastError());
  VIEO_HIP_CHECK(hipMemcpyAsync(e, d + o_e, 56 * (size_t)ne, hipMemcpyDeviceToHost, st));
  VIEO_HIP_CHECK(hipMemcpyAsync(Ji, d + o_ji, 392 * (size_t)ne, hipMemcpyDeviceToHost, st));
  VIEO_HIP_CHECK(hipMemcpyAsync(Jj, d + o_jj, 392 * (size_t)ne, hipMemcpyDeviceToHost, st));
  VIEO_HIP_CHECK(hipStreamSynchronize(st));
  return VIEO_OK;
}

extern "C" int vieo_pose_graph_solve(const vieo_pose_graph* g, double lambda, double* x, double* b, double* H_lower, int32_t* ok) {
  int rc;
  if ((rc = validate(g, false)) != VIEO_OK) return rc;
  if (!x || !b || !H_lower || !ok) {
    set_error("vieo_pose_graph_solve: null output");
    return VIEO_E_INVALID;
  }
  if ((rc = require_device()) != VIEO_OK) return rc;
  const int ne = g->n_edges, nk = g->n_kf, pd = g->fix_scale ? 6 : 7;
  PgPlan plan;
  pose_graph_plan_vertices(plan, nk, g->valid, g->fixed_kf, ne, g->edge_i, g->edge_j, pd);
  *ok = 1;
  if (plan.n_free == 0 || ne == 0) return VIEO_OK;
  pose_graph_plan_structure(plan, ne, g->edge_i, g->edge_j);
  static thread_local DevBuf buf;
  unsigned long long need = 0;
  if ((rc = check_capacity(plan, ne, nk, 0, buf.cap, &need)) != VIEO_OK) return rc;
  const int n = plan.n, T = plan.T;
  Arena A;
  const size_t o_scw = A.take(sizeof(Sim3) * nk), o_pri = A.take(sizeof(Sim3) * nk), o_meas = A.take(sizeof(Sim3) * ne);
  const size_t o_ei = A.take(4 * (size_t)ne), o_ej = A.take(4 * (size_t)ne), o_kind = A.take(4 * (size_t)ne);
  const size_t o_info = A.take(16 * (size_t)ne), o_blk = A.take(sizeof(EdgeBlk) * (size_t)ne), o_ok = A.take(64);
  PgSystem sys;
  sys.take(A, plan, true);
  if ((rc = buf.ensure(A.used)) != VIEO_OK) return rc;
  uint8_t* d = buf.as<uint8_t>();
  hipStream_t st = 0;
  VIEO_HIP_CHECK(hipMemcpyAsync(d + o_scw, g->Scw, sizeof(Sim3) * nk, hipMemcpyHostToDevice, st));
  VIEO_HIP_CHECK(hipMemcpyAsync(d + o_pri, g->Scw_prior, sizeof(Sim3) * nk, hipMemcpyHostToDevice, st));
  VIEO_HIP_CHECK(hipMemcpyAsync(d + o_ei, g->edge_i, 4 * (size_t)ne, hipMemcpyHostToDevice, st));
  VIEO_HIP_CHECK(hipMemcpyAsync(d + o_ej, g->edge_j, 4 * (size_t)ne, hipMemcpyHostToDevice, st));
  VIEO_HIP_CHECK(hipMemcpyAsync(d + o_kind, g->edge_kind, 4 * (size_t)ne, hipMemcpyHostToDevice, st));
  VIEO_HIP_CHECK(hipMemcpyAsync(d + o_info, g->edge_info, 16 * (size_t)ne, hipMemcpyHostToDevice, st));
  if ((rc = sys.upload(d, st)) != VIEO_OK) return rc;
  const int bs = alt_geometry() ? 128 : 256, epb = bs / LIN_LANES;
  k_pg_measure<<<(ne + bs - 1) / bs, bs, 0, st>>>(ne, (Sim3*)(d + o_scw), (Sim3*)(d + o_pri), (int*)(d + o_ei), (int*)(d + o_ej),
                                                  (int*)(d + o_kind), (Sim3*)(d + o_meas));
  k_pg_linearize<<<(ne + epb - 1) / epb, bs, 0, st>>>(ne, (Sim3*)(d + o_scw), (Sim3*)(d + o_meas), (int*)(d + o_ei),
                                                      (int*)(d + o_ej), (double*)(d + o_info), g->fix_scale != 0, nullptr, nullptr,
                                                      (EdgeBlk*)(d + o_blk), nullptr, nullptr);
  if ((rc = sys.assemble((EdgeBlk*)(d + o_blk), bs, st)) != VIEO_OK) return rc;
  if ((rc = sys.solve(lambda, (int*)(d + o_ok), st)) != VIEO_OK) return rc;
  VIEO_HIP_CHECK(hipGetLastError());
  // H as the tiles hold it, gathered on the host into the dense lower triangle
  std::vector<double> tiles(sys.tile_bytes / 8);
  int32_t flag = 0;
  VIEO_HIP_CHECK(hipMemcpyAsync(tiles.data(), sys.H(), sys.tile_bytes, hipMemcpyDeviceToHost, st));
  VIEO_HIP_CHECK(hipMemcpyAsync(x, sys.x(), 8 * (size_t)n, hipMemcpyDeviceToHost, st));
  VIEO_HIP_CHECK(hipMemcpyAsync(b, sys.b(), 8 * (size_t)n, hipMemcpyDeviceToHost, st));
  VIEO_HIP_CHECK(hipMemcpyAsync(&flag, d + o_ok, 4, hipMemcpyDeviceToHost, st));
  VIEO_HIP_CHECK(hipStreamSynchronize(st));
  *ok = flag != 0;
  memset(H_lower, 0, 8 * (size_t)n * n);
  for (int r = 0; r < T; r++)
    for (int c = plan.tfirst[r]; c <= r; c++) {
      const double* tile = tiles.data() + (size_t)(plan.tile_off[r] + c - plan.tfirst[r]) * TT;
      for (int i = 0; i < TS && r * TS + i < n; i++)
        for (int j = 0; j < TS && c * TS + j <= r * TS + i; j++) H_lower[(size_t)(r * TS + i) * n + c * TS + j] = tile[i * TS + j];
    }
  return VIEO_OK;
}

extern "C" int vieo_optimize_essential_graph(const vieo_pose_graph* g, vieo_pose_graph_result* out) {
  int rc;
  if ((rc = validate(g, true)) != VIEO_OK) return rc;
  if (!out || !out->Scw_opt || !out->Tcw || (g->n_mp && !out->Pw_out) || out->trace_cap < 0 || (out->trace_cap && !out->trace)) {
    set_error("vieo_optimize_essential_graph: null output");
    return VIEO_E_INVALID;
  }
  if ((rc = require_device()) != VIEO_OK) return rc;
  const int ne = g->n_edges, nk = g->n_kf, nmp = g->n_mp;
  const int pd = g->fix_scale ? 6 : 7;

  // ---- the symbolic part (pose_graph_plan.h): free vertices, the blocks of H, the tile envelope ----
  PgPlan plan;
  pose_graph_plan_vertices(plan, nk, g->valid, g->fixed_kf, ne, g->edge_i, g->edge_j, pd);
  const std::vector<int>& free_kf = plan.free_kf;
  const int n_free = plan.n_free, n = plan.n;
  const bool optimise = n_free > 0 && ne > 0 && g->n_iterations > 0;

  static thread_local DevBuf buf;
  static thread_local PinnedBuf pin;
  if (optimise) {
    pose_graph_plan_structure(plan, ne, g->edge_i, g->edge_j);
    unsigned long long need = 0;
    if ((rc = check_capacity(plan, ne, nk, nmp, buf.cap, &need)) != VIEO_OK) {
      if (rc == VIEO_E_CAPACITY) out->bytes_needed = need;
      return rc;
    }
  }

  // ---- device arena ----
  Arena A;
  const size_t o_scw = A.take(sizeof(Sim3) * nk), o_pri = A.take(sizeof(Sim3) * nk), o_est = A.take(sizeof(Sim3) * nk),
               o_bak = A.take(sizeof(Sim3) * nk), o_valid = A.take(nk), o_tcw = A.take(96 * (size_t)nk);
  const size_t o_meas = A.take(sizeof(Sim3) * ne), o_ei = A.take(4 * (size_t)ne), o_ej = A.take(4 * (size_t)ne),
               o_kind = A.take(4 * (size_t)ne), o_info = A.take(16 * (size_t)ne), o_chi = A.take(8 * (size_t)ne),
               o_blk = A.take(sizeof(EdgeBlk) * (size_t)ne);
  const size_t o_pw = A.take(12 * (size_t)nmp), o_ref = A.take(4 * (size_t)nmp), o_pwo = A.take(12 * (size_t)nmp),
               o_pwd = A.take(out->Pw_out_d ? 24 * (size_t)nmp : 0);
  const size_t o_free = A.take(4 * (size_t)n_free), o_sv = A.take(8 * (size_t)n_free), o_rec = A.take(64);
  PgSystem sys;
  sys.take(A, plan, optimise);
  if ((rc = buf.ensure(A.used)) != VIEO_OK) return rc;
  if ((rc = pin.ensure(64)) != VIEO_OK) return rc;
  uint8_t* d = buf.as<uint8_t>();
  hipStream_t st = 0;
#define PG_UP(off, src, bytes) \
  if (bytes) VIEO_HIP_CHECK(hipMemcpyAsync(d + (off), (src), (bytes), hipMemcpyHostToDevice, st))
  PG_UP(o_scw, g->Scw, sizeof(Sim3) * nk);
  PG_UP(o_pri, g->Scw_prior, sizeof(Sim3) * nk);
  PG_UP(o_est, g->Scw, sizeof(Sim3) * nk);
  PG_UP(o_bak, g->Scw, sizeof(Sim3) * nk);
  PG_UP(o_valid, g->valid, (size_t)nk);
  PG_UP(o_ei, g->edge_i, 4 * (size_t)ne);
  PG_UP(o_ej, g->edge_j, 4 * (size_t)ne);
  PG_UP(o_kind, g->edge_kind, 4 * (size_t)ne);
  PG_UP(o_info, g->edge_info, 16 * (size_t)ne);
  PG_UP(o_pw, g->Pw, 12 * (size_t)nmp);
  PG_UP(o_ref, g->ref_kf, 4 * (size_t)nmp);
  PG_UP(o_free, free_kf.data(), vbytes(free_kf));
#undef PG_UP
  if ((rc = sys.upload(d, st)) != VIEO_OK) return rc;
  Sim3 *dScw = (Sim3*)(d + o_scw), *dEst = (Sim3*)(d + o_est), *dBak = (Sim3*)(d + o_bak), *dMeas = (Sim3*)(d + o_meas);
  int *dEi = (int*)(d + o_ei), *dEj = (int*)(d + o_ej);
  double *dInfo = (double*)(d + o_info), *dChi = (double*)(d + o_chi), *dRec = (double*)(d + o_rec);
  double *dX = sys.x(), *dB = sys.b();
  int* dOk = (int*)(d + o_rec + 32);
  EdgeBlk* dBlk = (EdgeBlk*)(d + o_blk);
  const int bs = alt_geometry() ? 128 : 256, epb = bs / LIN_LANES;

  vieo_lba_result R;
  memset(&R, 0, sizeof R);
  int n_trace = 0;
  if (optimise) {
    k_pg_measure<<<(ne + bs - 1) / bs, bs, 0, st>>>(ne, dScw, (Sim3*)(d + o_pri), dEi, dEj, (int*)(d + o_kind), dMeas);
    LmMode mode;
    mode.full_ba = true, mode.user_lambda = true;
    WinLm lm;
    lm_start(lm, mode, g->n_iterations, 0, g->lambda_init, &R);
    double* rec = (double*)pin.p;
    for (;;) {
      const WinCtl ctl = lm_plan_round(lm, mode, false, 0);
      if (!ctl.flags) break;
      if (ctl.flags & LBA_RESTORE) VIEO_HIP_CHECK(hipMemcpyAsync(dEst, dBak, sizeof(Sim3) * nk, hipMemcpyDeviceToDevice, st));
      if (ctl.flags & LBA_BUILD) {
        k_pg_linearize<<<(ne + epb - 1) / epb, bs, 0, st>>>(ne, dEst, dMeas, dEi, dEj, dInfo, g->fix_scale != 0, nullptr, dChi, dBlk,
                                                            nullptr, nullptr);
        if (ctl.flags & LBA_BEGIN) k_pg_reduce<<<1, 256, 0, st>>>(dChi, ne, nullptr, 0, dOk, dRec, 0);
        if ((rc = sys.assemble(dBlk, bs, st)) != VIEO_OK) return rc;
      }
      if (!(ctl.flags & LBA_TRIAL)) continue;
      // (H + lambda I) x = b
      if ((rc = sys.solve(ctl.lambda, dOk, st)) != VIEO_OK) return rc;
      k_pg_update<<<(n_free + bs - 1) / bs, bs, 0, st>>>(n_free, (int*)(d + o_free), pd, dX, dB, ctl.lambda, dEst, dBak,
                                                         (double*)(d + o_sv));
      k_pg_errors<<<(ne + bs - 1) / bs, bs, 0, st>>>(ne, dEst, dMeas, dEi, dEj, dInfo, dChi);
      k_pg_reduce<<<1, 256, 0, st>>>(dChi, ne, (double*)(d + o_sv), n_free, dOk, dRec, 1);
      VIEO_HIP_CHECK(hipGetLastError());
      VIEO_HIP_CHECK(hipMemcpyAsync(rec, dRec, 32, hipMemcpyDeviceToHost, st));
      VIEO_HIP_CHECK(hipStreamSynchronize(st));
      WinOut wo;
      memset(&wo, 0, sizeof wo);
      wo.chi0 = rec[0], wo.chi2 = rec[1], wo.scale_l = rec[2], wo.ok = rec[3] != 0.0, wo.np = n_free, wo.lambda = ctl.lambda;
      const double before = (ctl.flags & LBA_BEGIN) ? wo.chi0 : lm.currentChi;
      lm_digest_trial(lm, mode, ctl.flags, wo, nullptr, false);
      if (n_trace < out->trace_cap)
        out->trace[n_trace++] = vieo_pg_trial{before, wo.chi2, ctl.lambda, lm.need_restore ? 0 : 1, wo.ok};
    }
  }
  const int nt = std::max(nk, nmp);
  k_pg_finish<<<(nt + bs - 1) / bs, bs, 0, st>>>(nk, d + o_valid, dEst, dScw, (double*)(d + o_tcw), nmp, (float*)(d + o_pw),
                                                 (int*)(d + o_ref), (float*)(d + o_pwo), out->Pw_out_d ? (double*)(d + o_pwd) : nullptr);
  VIEO_HIP_CHECK(hipGetLastError());
  VIEO_HIP_CHECK(hipMemcpyAsync(out->Scw_opt, dEst, sizeof(Sim3) * nk, hipMemcpyDeviceToHost, st));
  VIEO_HIP_CHECK(hipMemcpyAsync(out->Tcw, d + o_tcw, 96 * (size_t)nk, hipMemcpyDeviceToHost, st));
  if (nmp) VIEO_HIP_CHECK(hipMemcpyAsync(out->Pw_out, d + o_pwo, 12 * (size_t)nmp, hipMemcpyDeviceToHost, st));
  if (nmp && out->Pw_out_d) VIEO_HIP_CHECK(hipMemcpyAsync(out->Pw_out_d, d + o_pwd, 24 * (size_t)nmp, hipMemcpyDeviceToHost, st));
  VIEO_HIP_CHECK(hipStreamSynchronize(st));
  out->status = VIEO_OK;
  out->n_unknowns = optimise ? n : 0;
  out->lm_iterations = R.lm_iterations, out->lm_trials = R.lm_trials;
  out->chi2_initial = R.chi2_initial, out->chi2_final = R.chi2_final;
  out->n_trace = n_trace;
  out->bytes_needed = 0;
  return VIEO_OK;
}
