// pose_graph_plan.h -- the symbolic part of the pose graph's tile-sparse LDL^T (pose_graph.hip): which key frames are
// unknowns, the 7 x 7 blocks of H with their edges in edge order, the tile envelope and the row list of every tile
// column.  Host-only C++ (no HIP): the tests compile it with g++.
//
// A vertex is free when it is valid, not the fixed one and has an edge (g2o's active set); free vertex f owns the
// unknowns f pd .. f pd + pd - 1, in key-frame order.  H is kept as 64 x 64 tiles of the lower triangle inside the row
// envelope: tile row r holds tile columns tfirst[r] .. r, tfirst[r] the leftmost tile a block of the row touches.  A
// right-looking LDL^T fills nothing outside that envelope.  The right-hand side is tile row T over columns 0 .. T - 1.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace vieo {

static const int kPgTile = 64;

struct PgAsmItem {  // one 7 x 7 block of H (and, for a diagonal block, 7 entries of b): a sum over refs[begin, end)
  int diag;         // 1: diagonal block of a vertex (ref flag: the vertex is the edge's vertex 1); 0: off-diagonal block
                    // (ref flag: the edge's vertex 0 is the block's COLUMN vertex, its Hij enters transposed)
  int rbase, cbase;
  int begin, end;
};

struct PgPlan {
  int pd = 0, n_free = 0, n = 0, T = 0;  // unknowns per vertex, free vertices, unknowns, tile rows of H
  long long n_ll = 0, tiles = 0;         // n before it is narrowed; tiles of H and of the right-hand side's row
  std::vector<int> col_of, free_kf;      // [n_kf] ordinal of a free key frame or -1; [n_free] its key frame
  std::vector<PgAsmItem> items;          // diagonal blocks in vertex order, then off-diagonal blocks by (row, column) vertex
  std::vector<int> refs;                 // edge << 1 | flag, per item in edge order
  std::vector<int> tfirst, tile_off;     // [T + 1] first tile column of a tile row; [T + 2] prefix sum of the rows' tile counts
  std::vector<int> list_off, rows;       // [T + 1], [list_off[T]]: per tile column k the tile rows below it that reach it,
                                         // ascending, then T (the right-hand side's)
};

// the free vertices alone: col_of, free_kf, n_free, n, T
inline void pose_graph_plan_vertices(PgPlan& P, int n_kf, const uint8_t* valid, int fixed_kf, int n_edges, const int* edge_i,
                                     const int* edge_j, int pd) {
  P = PgPlan();
  P.pd = pd;
  std::vector<int> deg(n_kf, 0);
  P.col_of.assign(n_kf, -1);
  for (int e = 0; e < n_edges; e++) deg[edge_i[e]]++, deg[edge_j[e]]++;
  for (int k = 0; k < n_kf; k++)
    if (valid[k] && k != fixed_kf && deg[k] > 0) P.col_of[k] = (int)P.free_kf.size(), P.free_kf.push_back(k);
  P.n_free = (int)P.free_kf.size();
  P.n_ll = (long long)P.n_free * pd;
  P.n = (int)P.n_ll, P.T = (P.n + kPgTile - 1) / kPgTile;
}

// the blocks, the envelope and the row lists of a plan whose vertices are set (n_free > 0)
inline void pose_graph_plan_structure(PgPlan& P, int n_edges, const int* edge_i, const int* edge_j) {
  const int TS = kPgTile, pd = P.pd, n_free = P.n_free, T = P.T, ne = n_edges;
  const std::vector<int>& col_of = P.col_of;
  std::vector<PgAsmItem>& items = P.items;
  std::vector<int>&refs = P.refs, &tfirst = P.tfirst, &tile_off = P.tile_off, &list_off = P.list_off, &rows = P.rows;
  // diagonal blocks: CSR vertex -> incident edges, in edge order
  std::vector<int> vstart(n_free + 1, 0);
  for (int e = 0; e < ne; e++) {
    if (col_of[edge_i[e]] >= 0) vstart[col_of[edge_i[e]] + 1]++;
    if (col_of[edge_j[e]] >= 0) vstart[col_of[edge_j[e]] + 1]++;
  }
  for (int f = 0; f < n_free; f++) vstart[f + 1] += vstart[f];
  refs.resize(vstart[n_free]);
  std::vector<int> fill(vstart.begin(), vstart.end() - 1);
  for (int e = 0; e < ne; e++) {
    if (col_of[edge_i[e]] >= 0) refs[fill[col_of[edge_i[e]]]++] = e << 1;
    if (col_of[edge_j[e]] >= 0) refs[fill[col_of[edge_j[e]]]++] = e << 1 | 1;
  }
  for (int f = 0; f < n_free; f++) items.push_back(PgAsmItem{1, f * pd, f * pd, vstart[f], vstart[f + 1]});
  // off-diagonal blocks (row vertex: the later column), their edges in edge order
  struct OffRef {
    long long key;
    int ref;
  };
  std::vector<OffRef> off;
  for (int e = 0; e < ne; e++) {
    const int ci = col_of[edge_i[e]], cj = col_of[edge_j[e]];
    if (ci < 0 || cj < 0) continue;
    const int hi = std::max(ci, cj), lo = std::min(ci, cj);
    off.push_back(OffRef{(long long)hi * n_free + lo, e << 1 | (ci < cj ? 1 : 0)});
  }
  std::stable_sort(off.begin(), off.end(), [](const OffRef& a, const OffRef& b) { return a.key < b.key; });
  for (size_t k = 0; k < off.size();) {
    size_t k1 = k;
    const int begin = (int)refs.size();
    while (k1 < off.size() && off[k1].key == off[k].key) refs.push_back(off[k1++].ref);
    items.push_back(PgAsmItem{0, (int)(off[k].key / n_free) * pd, (int)(off[k].key % n_free) * pd, begin, (int)refs.size()});
    k = k1;
  }
  // envelope: first tile column of every tile row; the right-hand side is tile row T over columns 0 .. T-1
  tfirst.resize(T + 1);
  for (int r = 0; r < T; r++) tfirst[r] = r;
  tfirst[T] = 0;
  for (const PgAsmItem& I : items)
    for (int tr = I.rbase / TS; tr <= (I.rbase + pd - 1) / TS; tr++) tfirst[tr] = std::min(tfirst[tr], I.cbase / TS);
  tile_off.resize(T + 2);
  tile_off[0] = 0;
  long long tiles = 0;
  for (int r = 0; r <= T; r++) {
    tile_off[r] = (int)tiles;
    tiles += r < T ? r - tfirst[r] + 1 : T;
    if (tiles > 0x3fffffff) break;
  }
  tile_off[T + 1] = (int)tiles;
  P.tiles = tiles;
  // row list of every tile column k: the tile rows below k whose envelope reaches it, then the right-hand side's
  list_off.assign(T + 1, 0);
  for (int r = 0; r < T; r++)
    for (int k = tfirst[r]; k < r; k++) list_off[k + 1]++;
  for (int k = 0; k < T; k++) list_off[k + 1] += list_off[k] + 1;
  rows.resize(list_off[T]);
  std::vector<int> at(list_off.begin(), list_off.end() - 1);
  for (int r = 0; r < T; r++)
    for (int k = tfirst[r]; k < r; k++) rows[at[k]++] = r;
  for (int k = 0; k < T; k++) rows[at[k]++] = T;
}

}  // namespace vieo
