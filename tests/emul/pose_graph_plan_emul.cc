// The symbolic part of the pose graph's solve (vieo_slam_amd/csrc/pose_graph_plan.h) behind a C interface, for
// tests/test_pose_graph_plan.py.  Test only.
#include "../../vieo_slam_amd/csrc/pose_graph_plan.h"

static vieo::PgPlan g_plan;

static const std::vector<int>& pick(int w) {
  const vieo::PgPlan& P = g_plan;
  const std::vector<int>* l[] = {&P.col_of, &P.free_kf, &P.refs, &P.tfirst, &P.tile_off, &P.list_off, &P.rows};
  return *l[w];
}

extern "C" {

void pgp_build(int n_kf, const uint8_t* valid, int fixed_kf, int n_edges, const int* ei, const int* ej, int pd) {
  vieo::pose_graph_plan_vertices(g_plan, n_kf, valid, fixed_kf, n_edges, ei, ej, pd);
  if (g_plan.n_free > 0 && n_edges > 0) vieo::pose_graph_plan_structure(g_plan, n_edges, ei, ej);
}
void pgp_header(long long* h) {
  h[0] = g_plan.pd, h[1] = g_plan.n_free, h[2] = g_plan.n, h[3] = g_plan.T, h[4] = g_plan.tiles, h[5] = (long long)g_plan.items.size();
}
int pgp_len(int w) { return (int)pick(w).size(); }
void pgp_get(int w, int* out) {
  for (size_t i = 0; i < pick(w).size(); i++) out[i] = pick(w)[i];
}
void pgp_items(int* out) {  // diag, rbase, cbase, begin, end
  for (size_t i = 0; i < g_plan.items.size(); i++) {
    const vieo::PgAsmItem& I = g_plan.items[i];
    out[5 * i] = I.diag, out[5 * i + 1] = I.rbase, out[5 * i + 2] = I.cbase, out[5 * i + 3] = I.begin, out[5 * i + 4] = I.end;
  }
}

}  // extern "C"
