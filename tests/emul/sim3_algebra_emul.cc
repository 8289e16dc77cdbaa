// The Sim3 algebra of the pose graph (vieo_slam_amd/csrc/sim3_device.h) and the state functions, Huber and the small
// LDL^T of OptimizeSim3 (sim3_optimize_device.h) compiled for the host, one call per family over a list of cases, with
// the branch taps of S3_TAP (kTapSlots doubles a case).  The second evaluator of
// tests/test_sim3_algebra.py beside tests/hip_unit/sim3_algebra_test.hip.  Test only.
#include <cstring>

static const int kTapSlots = 12;
static thread_local double* g_tap = nullptr;
#define S3_TAP(slot, value) \
  if (g_tap) g_tap[slot] = (value);

#include "../../vieo_slam_amd/csrc/sim3_device.h"
#include "../../vieo_slam_amd/csrc/sim3_optimize_device.h"

using namespace vieo;
static_assert(sizeof(Sim3) == 64, "Sim3 is eight doubles");
static_assert(sizeof(S3oState) == 64, "S3oState is eight doubles");

extern "C" {

int emul_s3a_tap_slots() { return kTapSlots; }

void emul_s3a_quat_to_mat(int n, const double* q, double* R) {
  for (int i = 0; i < n; i++) s3_quat_to_mat(q + 4 * i, R + 9 * i);
}
void emul_s3a_mat_to_quat(int n, const double* R, double* q, double* tap) {
  for (int i = 0; i < n; i++) {
    g_tap = tap + (size_t)kTapSlots * i;
    s3_mat_to_quat(R + 9 * i, q + 4 * i);
  }
  g_tap = nullptr;
}
void emul_s3a_quat_rot(int n, const double* q, const double* v, double* o) {
  for (int i = 0; i < n; i++) s3_quat_rot(q + 4 * i, v + 3 * i, o + 3 * i);
}
void emul_s3a_mul(int n, const Sim3* a, const Sim3* b, Sim3* o) {
  for (int i = 0; i < n; i++) o[i] = s3_mul(a[i], b[i]);
}
void emul_s3a_inverse(int n, const Sim3* a, Sim3* o) {
  for (int i = 0; i < n; i++) o[i] = s3_inverse(a[i]);
}
void emul_s3a_map(int n, const Sim3* a, const double* p, double* o) {
  for (int i = 0; i < n; i++) s3_map(a[i], p + 3 * i, o + 3 * i);
}
void emul_s3a_exp(int n, const double* u, Sim3* o, double* tap) {
  for (int i = 0; i < n; i++) {
    g_tap = tap + (size_t)kTapSlots * i;
    o[i] = s3_exp(u + 7 * i);
  }
  g_tap = nullptr;
}
void emul_s3a_log(int n, const Sim3* S, double* o, double* tap) {
  for (int i = 0; i < n; i++) {
    g_tap = tap + (size_t)kTapSlots * i;
    s3_log(S[i], o + 7 * i);
  }
  g_tap = nullptr;
}
void emul_s3a_edge_error(int n, const Sim3* C, const Sim3* Si, const Sim3* Sj, double* o, double* tap) {
  for (int i = 0; i < n; i++) {
    g_tap = tap + (size_t)kTapSlots * i;
    s3_edge_error(C[i], Si[i], Sj[i], o + 7 * i);
  }
  g_tap = nullptr;
}

// ---- sim3_optimize_device.h: a state is p[3], q[4], s
void emul_s3a_quat_normalize(int n, const double* q, double* o) {
  for (int i = 0; i < n; i++) {
    for (int k = 0; k < 4; k++) o[4 * i + k] = q[4 * i + k];
    s3o_quat_normalize(o + 4 * i);
  }
}
void emul_s3a_state_from_sim3(int n, const double* Rts, S3oState* o) {  // Rts = R12[9], t12[3], s12
  for (int i = 0; i < n; i++) s3o_state_from_sim3(Rts + 13 * i, Rts + 13 * i + 9, Rts[13 * i + 12], o[i]);
}
void emul_s3a_state_to_sim3(int n, const S3oState* st, double* o) {  // o = R12[9], t12[3], s12
  for (int i = 0; i < n; i++) s3o_state_to_sim3(st[i], o + 13 * i, o + 13 * i + 9, o + 13 * i + 12);
}
void emul_s3a_inc_small(int n, const S3oState* st, const double* d, S3oState* o, double* tap) {  // d = the increment[7], fix_scale
  for (int i = 0; i < n; i++) {
    g_tap = tap + (size_t)kTapSlots * i;
    o[i] = st[i];
    s3o_inc_small(o[i], d + 8 * i, d[8 * i + 7] != 0.0);
  }
  g_tap = nullptr;
}
// a camera as the tests pass it: model, num_k, fx, fy, cx, cy, k[8], Rcb[9], tcb[3] (26 doubles)
static CamD cam_of(const double* c) {
  CamD d;
  d.model = (int)c[0], d.num_k = (int)c[1];
  d.fx = c[2], d.fy = c[3], d.cx = c[4], d.cy = c[5], d.bf = 0;
  for (int i = 0; i < 8; i++) d.k[i] = c[6 + i];
  for (int i = 0; i < 9; i++) d.Rcb[i] = c[14 + i];
  for (int i = 0; i < 3; i++) d.tcb[i] = c[23 + i];
  return d;
}
// in = mode, camera, q[4], p[3], s, X[3], obs[2]; o = e[2] and J[14] of the call with J, e[2] of the call without
void emul_s3a_edge(int n, const double* in, const double* cams, double* o) {
  for (int i = 0; i < n; i++) {
    const double* a = in + 15 * i;
    const CamD c = cam_of(cams + 26 * (int)a[1]);
    double Rwb[9];
    s3_quat_to_mat(a + 2, Rwb);
    if (a[0] == 1.0) {
      s3o_edge<1>(c, Rwb, a + 6, a[9], a + 10, a + 13, o + 18 * i, o + 18 * i + 2);
      s3o_edge<1>(c, Rwb, a + 6, a[9], a + 10, a + 13, o + 18 * i + 16, nullptr);
    } else {
      s3o_edge<2>(c, Rwb, a + 6, a[9], a + 10, a + 13, o + 18 * i, o + 18 * i + 2);
      s3o_edge<2>(c, Rwb, a + 6, a[9], a + 10, a + 13, o + 18 * i + 16, nullptr);
    }
  }
}
// in = e[2], J[14], info, delta, dsqr; o = the 36 accumulators from zero, s3o_chi2
void emul_s3a_add_edge(int n, const double* in, double* o) {
  for (int i = 0; i < n; i++) {
    const double* a = in + 19 * i;
    double* acc = o + 37 * i;
    for (int k = 0; k < 36; k++) acc[k] = 0;
    const double chi2 = s3o_chi2(a, a[16]);
    s3o_add_edge(a, a + 2, a[16], chi2, a[17], a[18], acc);
    acc[36] = chi2;
  }
}
void emul_s3a_huber(int n, const double* in, double* o) {  // in = e2, delta, dsqr
  for (int i = 0; i < n; i++) s3o_huber(in[3 * i], in[3 * i + 1], in[3 * i + 2], o + 2 * i, o + 2 * i + 1);
}
void emul_s3a_ldlt(int n, const double* in, double* o) {  // in = acc[36], lambda, N; o = ok, x[7] (x starts as a guard)
  for (int i = 0; i < n; i++) {
    const double* a = in + 38 * i;
    double* x = o + 8 * i + 1;
    for (int k = 0; k < 7; k++) x[k] = -7.0;
    o[8 * i] = a[37] == 6.0 ? s3o_ldlt_solve<6>(a, a[36], x) : s3o_ldlt_solve<7>(a, a[36], x);
  }
}

}  // extern "C"
