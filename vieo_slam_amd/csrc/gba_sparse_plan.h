// gba_sparse_plan.h -- symbolic plan of the full BA's tile-sparse LDL^T (solver class 3 of lba.hip; the kernels:
// lba_schur_device.h, lba_solve_device.h).
// Host-only C++ (no HIP): the tests compile it with g++.
//
// The full BA's reduced pose system is factorised like the dense tiled solve (k_big_*): right-looking over 64-column
// panels of the lower triangle of the bordered matrix [H b; b^T .] -- the right-hand side is row n -- with the columns in
// k_lba_begin's order.  A 64 x 64 tile that is structurally zero only ever contributes exact zeros there, so storing and
// touching only the tiles of the symbolic fill pattern computes the same numbers.  The plan lists:
//   * the non-zero tiles (bi <= bj) of the visual Schur product on k_lba_schur's 6 nf + sco grid (+ the b_l column);
//   * the tiles of the reduced system's lower triangle closed under tile-level elimination, column by column (diagonal
//     tile first): a tile's position in that order is its slot in the pool (4096 doubles each);
//   * the same tiles row by row (column ascending, diagonal last): the back-substitution's rows;
//   * for every panel k, its update targets (i, j) with the slots of (i, k), (j, k) and (i, j).
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

namespace vieo {

static const int kGbaTile = 64, kGbaTileElems = kGbaTile * kGbaTile;

struct GbaSparsePlan {
  int pd = 0, sco = 0, nf = 0;  // unknowns per key frame (6 / 15), scale vertex, free key frames with a column
  int n = 0, nt = 0;            // unknowns pd nf + sco; tile rows of the bordered system (n + 1 rows)
  int vrb = 0, vcb = 0;         // visual Schur product: row / column tiles of the 6 nf + sco grid (+ the b_l column)
  std::vector<int> col_of;      // [n_kf] column ordinal of a key frame, -1 = none (k_lba_begin's rule)
  // visual Schur product: non-zero tiles (bi <= bj), row by row, bj ascending; the diagonal / off-diagonal ones
  std::vector<int> sch_ptr, sch_i, sch_j, sch_diag, sch_off;
  // reduced system: stored tiles column by column (diagonal first); slot = position
  std::vector<int> col_ptr, tile_i, tile_j;
  // the same tiles row by row (column ascending, diagonal last): column tile and slot
  std::vector<int> row_ptr, row_j, row_tile;
  // update targets of panel k: upd[5 u ..] = i, j, slot (i, k), slot (j, k), slot (i, j) for u in [upd_ptr[k], upd_ptr[k + 1])
  std::vector<int> upd_ptr, upd;
  int max_col = 0, max_upd = 0, max_row = 0;  // largest tile count below a diagonal / update list / row (launch grids)

  size_t n_tiles() const { return tile_i.size(); }
  size_t n_sch_tiles() const { return sch_i.size(); }
  size_t pool_bytes() const { return n_tiles() * kGbaTileElems * sizeof(double); }
  size_t schur_bytes(int ksplit) const { return (size_t)ksplit * n_sch_tiles() * kGbaTileElems * sizeof(double); }
  size_t panel_bytes() const { return (size_t)nt * kGbaTile * kGbaTile * sizeof(double); }  // W of a panel, [nt 64][64]
  size_t list_ints() const {
    return sch_ptr.size() + sch_i.size() + sch_j.size() + sch_diag.size() + sch_off.size() + col_ptr.size() +
           tile_i.size() + tile_j.size() + row_ptr.size() + row_j.size() + row_tile.size() + upd_ptr.size() + upd.size();
  }
  // device bytes of the tile-sparse solve: pool + Schur partials + panel + the plan's lists
  size_t bytes(int ksplit) const { return pool_bytes() + schur_bytes(ksplit) + panel_bytes() + list_ints() * sizeof(int); }
};

// n_kf key frames (fixed[k] != 0: fixed); observations (kf | camera << 24, mp) -- the camera bits are masked off, out of
// range entries are ignored; n_pair inertial / encoder pair edges (kf_i, kf_j); pd = 6 or 15; sco: the scale vertex.
inline void gba_sparse_plan(GbaSparsePlan& P, int n_kf, const int* fixed, int n_obs, const int* obs_kf, const int* obs_mp,
                            int n_mp, int n_pair, const int* pair_i, const int* pair_j, int pd, int sco) {
  const int T = kGbaTile;
  P = GbaSparsePlan();
  P.pd = pd, P.sco = sco ? 1 : 0;
  // columns: free and active key frames, or every free key frame with 15-dim vertices (k_lba_begin)
  std::vector<char> act(n_kf > 0 ? n_kf : 0, 0);
  std::vector<int> okf(n_obs > 0 ? n_obs : 0, -1);
  for (int i = 0; i < n_obs; i++) {
    const int k = obs_kf[i] & 0xFFFFFF, m = obs_mp[i];
    if (obs_kf[i] < 0 || k >= n_kf || m < 0 || m >= n_mp) continue;
    okf[i] = k, act[k] = 1;
  }
  if (pd == 6)
    for (int e = 0; e < n_pair; e++)
      if (pair_i[e] >= 0 && pair_i[e] < n_kf && pair_j[e] >= 0 && pair_j[e] < n_kf) act[pair_i[e]] = act[pair_j[e]] = 1;
  P.col_of.assign(n_kf > 0 ? n_kf : 0, -1);
  for (int k = 0; k < n_kf; k++)
    if (!fixed[k] && (act[k] || pd == 15)) P.col_of[k] = P.nf++;
  const int nf = P.nf, npv = 6 * nf + P.sco;
  P.n = pd * nf + P.sco;
  P.nt = (P.n + 1 + T - 1) / T;
  P.vrb = (npv + T - 1) / T, P.vcb = (npv + T) / T;
  // observers (columns) of every point, and which points have an observation at all
  std::vector<std::pair<int, int>> mo;  // (point, column)
  std::vector<char> mp_act(n_mp > 0 ? n_mp : 0, 0);
  for (int i = 0; i < n_obs; i++) {
    if (okf[i] < 0) continue;
    mp_act[obs_mp[i]] = 1;
    if (P.col_of[okf[i]] >= 0) mo.emplace_back(obs_mp[i], P.col_of[okf[i]]);
  }
  std::sort(mo.begin(), mo.end());
  mo.erase(std::unique(mo.begin(), mo.end()), mo.end());
  // ---- visual Schur product: tile (bi, bj) of BB BB^T is non-zero where a point is seen from both row ranges
  const int vrb = P.vrb, vcb = P.vcb, nt = P.nt, n = P.n;
  std::vector<char> S((size_t)vrb * vcb, 0);
  std::vector<char> R((size_t)nt * nt, 0);  // lower triangle of the reduced system's tiles, R[I nt + J], I >= J
  auto markR = [&](int r0, int h, int c0, int w) {  // entries [r0, r0 + h) x [c0, c0 + w) and their transposes
    for (int I = r0 / T; I <= (r0 + h - 1) / T; I++)
      for (int J = c0 / T; J <= (c0 + w - 1) / T; J++) R[(size_t)std::max(I, J) * nt + std::min(I, J)] = 1;
  };
  std::vector<int> tiles, cols;
  const int sc_tile = (npv - 1) / T;
  for (size_t s = 0; s < mo.size();) {
    size_t e = s;
    while (e < mo.size() && mo[e].first == mo[s].first) e++;
    tiles.clear(), cols.clear();
    for (size_t q = s; q < e; q++) {
      const int a = mo[q].second;
      cols.push_back(a);
      tiles.push_back(6 * a / T), tiles.push_back((6 * a + 5) / T);
    }
    if (P.sco) tiles.push_back(sc_tile);
    std::sort(tiles.begin(), tiles.end());
    tiles.erase(std::unique(tiles.begin(), tiles.end()), tiles.end());
    for (size_t x = 0; x < tiles.size(); x++)
      for (size_t y = x; y < tiles.size(); y++) S[(size_t)tiles[x] * vcb + tiles[y]] = 1;
    // reduced system: the PR x PR blocks of every covisible pair (k_lba_assemble: rows pd a + 0..5)
    for (size_t x = 0; x < cols.size(); x++)
      for (size_t y = x + 1; y < cols.size(); y++) markR(pd * cols[x], 6, pd * cols[y], 6);
    s = e;
  }
  if (P.sco)  // points seen from fixed key frames only still reach the scale vertex's own entry
    for (int m = 0; m < n_mp; m++)
      if (mp_act[m]) {
        S[(size_t)sc_tile * vcb + sc_tile] = 1;
        break;
      }
  for (int bi = 0; bi < vrb; bi++) S[(size_t)bi * vcb + vcb - 1] = 1;  // the b_l column
  P.sch_ptr.assign(vrb + 1, 0);
  for (int bi = 0; bi < vrb; bi++) {
    for (int bj = bi; bj < vcb; bj++)
      if (S[(size_t)bi * vcb + bj]) {
        (bi == bj ? P.sch_diag : P.sch_off).push_back((int)P.sch_i.size());
        P.sch_i.push_back(bi), P.sch_j.push_back(bj);
      }
    P.sch_ptr[bi + 1] = (int)P.sch_i.size();
  }
  // ---- reduced system: diagonal blocks, pair edges, the scale row, the right-hand-side row, every diagonal tile
  for (int a = 0; a < nf; a++) markR(pd * a, pd, pd * a, pd);
  for (int e = 0; e < n_pair; e++) {
    const int i = pair_i[e], j = pair_j[e];
    if (i < 0 || i >= n_kf || j < 0 || j >= n_kf) continue;
    const int a = P.col_of[i], b = P.col_of[j];
    if (a >= 0 && b >= 0) markR(pd * a, pd, pd * b, pd);
  }
  if (P.sco)
    for (int J = 0; J <= (n - 1) / T; J++) R[(size_t)((n - 1) / T) * nt + J] = 1;
  for (int J = 0; J < nt; J++) R[(size_t)(n / T) * nt + J] = 1, R[(size_t)J * nt + J] = 1;
  // ---- fill: eliminating tile column k couples every pair of its row tiles
  std::vector<int> rows;
  for (int k = 0; k < nt; k++) {
    rows.clear();
    for (int I = k + 1; I < nt; I++)
      if (R[(size_t)I * nt + k]) rows.push_back(I);
    for (size_t x = 0; x < rows.size(); x++)
      for (size_t y = 0; y <= x; y++) R[(size_t)rows[x] * nt + rows[y]] = 1;
  }
  // ---- slots (column-major), row lists, update lists
  std::vector<int> slot((size_t)nt * nt, -1);
  P.col_ptr.assign(nt + 1, 0);
  for (int J = 0; J < nt; J++) {
    for (int I = J; I < nt; I++)
      if (R[(size_t)I * nt + J]) {
        slot[(size_t)I * nt + J] = (int)P.tile_i.size();
        P.tile_i.push_back(I), P.tile_j.push_back(J);
      }
    P.col_ptr[J + 1] = (int)P.tile_i.size();
    P.max_col = std::max(P.max_col, P.col_ptr[J + 1] - P.col_ptr[J] - 1);
  }
  P.row_ptr.assign(nt + 1, 0);
  for (int I = 0; I < nt; I++) {
    for (int J = 0; J <= I; J++)
      if (R[(size_t)I * nt + J]) P.row_j.push_back(J), P.row_tile.push_back(slot[(size_t)I * nt + J]);
    P.row_ptr[I + 1] = (int)P.row_j.size();
    P.max_row = std::max(P.max_row, P.row_ptr[I + 1] - P.row_ptr[I] - 1);
  }
  P.upd_ptr.assign(nt + 1, 0);
  for (int k = 0; k < nt; k++) {
    const int c0 = P.col_ptr[k] + 1, c1 = P.col_ptr[k + 1];  // the tiles below the diagonal one
    for (int x = c0; x < c1; x++)
      for (int y = c0; y <= x; y++) {
        const int i = P.tile_i[x], j = P.tile_i[y];
        const int u[5] = {i, j, x, y, slot[(size_t)i * nt + j]};
        P.upd.insert(P.upd.end(), u, u + 5);
      }
    P.upd_ptr[k + 1] = (int)(P.upd.size() / 5);
    P.max_upd = std::max(P.max_upd, P.upd_ptr[k + 1] - P.upd_ptr[k]);
  }
}

}  // namespace vieo
