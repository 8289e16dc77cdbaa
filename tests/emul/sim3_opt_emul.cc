// The lane functions of the OptimizeSim3 kernel (vieo_slam_amd/csrc/sim3_optimize_device.h) compiled for the host: the
// edges with their Jacobians, the retraction, the LDL^T and the whole visit with a functor of 1 or 64 lanes (64: the
// lane <-> correspondence map of the kernel and the adjacent-pair tree of its DPP sums).  Test only.
#include <cstring>
#include <vector>

#include "../../vieo_slam_amd/csrc/sim3_optimize_device.h"

using namespace vieo;

namespace {

// a camera as the tests pass it: model, num_k, fx, fy, cx, cy, k[8], Rcb[9], tcb[3] (26 doubles)
CamD cam_of(const double* c) {
  CamD d;
  d.model = (int)c[0], d.num_k = (int)c[1];
  d.fx = c[2], d.fy = c[3], d.cx = c[4], d.cy = c[5], d.bf = 0;
  for (int i = 0; i < 8; i++) d.k[i] = c[6 + i];
  for (int i = 0; i < 9; i++) d.Rcb[i] = c[14 + i];
  for (int i = 0; i < 3; i++) d.tcb[i] = c[23 + i];
  return d;
}

template <int NL>
struct HostLanes {
  bool leader() const { return true; }
  template <int N, class F>
  void run(F f, double* out) {
    static double part[NL][N];
    for (int l = 0; l < NL; l++) f(l, NL, part[l]);
    for (int w = 1; w < NL; w *= 2)
      for (int l = 0; l < NL; l += 2 * w)
        for (int i = 0; i < N; i++) part[l][i] += part[l + w][i];
    for (int i = 0; i < N; i++) out[i] = part[0][i];
  }
};

}  // namespace

extern "C" {

int emul_s3o_corr_size() { return (int)sizeof(S3oCorr); }

void emul_s3o_edge(int mode, const double* cam, const double* q, const double* p, double s, const double* X, const double* obs,
                   double* e, double* J) {
  const CamD c = cam_of(cam);
  double Rwb[9];
  s3_quat_to_mat(q, Rwb);
  if (mode == 1)
    s3o_edge<1>(c, Rwb, p, s, X, obs, e, J);
  else
    s3o_edge<2>(c, Rwb, p, s, X, obs, e, J);
}

// st = p[3], q[4], s
void emul_s3o_from_sim3(const double* R12, const double* t12, double s12, double* st) {
  S3oState S;
  s3o_state_from_sim3(R12, t12, s12, S);
  memcpy(st, &S, sizeof(S));
}
void emul_s3o_to_sim3(const double* st, double* R12, double* t12, double* s12) {
  S3oState S;
  memcpy(&S, st, sizeof(S));
  s3o_state_to_sim3(S, R12, t12, s12);
}
void emul_s3o_inc_small(double* st, const double* d, int fix_scale) {
  S3oState S;
  memcpy(&S, st, sizeof(S));
  s3o_inc_small(S, d, fix_scale != 0);
  memcpy(st, &S, sizeof(S));
}
int emul_s3o_ldlt(const double* acc, double lambda, int n, double* x) {
  return n == 6 ? s3o_ldlt_solve<6>(acc, lambda, x) : s3o_ldlt_solve<7>(acc, lambda, x);
}

// the whole visit.  ints: n_inliers, n_bad, returned0, n_trials, iterations[2], trials[2]
void emul_s3o_visit(int n_lanes, int n, const void* corr, int n_cams, const double* cams, const double* st_in, float th2,
                    int fix_scale, double* st_out, int32_t* ints, int32_t* erased, double* chi_check, double* trace) {
  std::vector<CamD> C(n_cams);
  for (int i = 0; i < n_cams; i++) C[i] = cam_of(cams + 26 * i);
  std::vector<double> chi(2 * (size_t)n + 2);
  S3oVisit P;
  memset(&P, 0, sizeof(P));
  memcpy(&P.st, st_in, sizeof(P.st));
  const float delta = std::sqrt(th2);
  P.th2 = (double)th2, P.delta = (double)delta, P.dsqr = P.delta * P.delta;
  P.first = 0, P.n = n, P.fix_scale = fix_scale != 0;
  S3oView V;
  V.corr = (const S3oCorr*)corr, V.cams = C.data(), V.n = n;
  V.chi = chi.data(), V.chi_check = chi_check, V.erased = erased, V.trace = trace;
  memset(erased, 0, sizeof(int32_t) * n);
  memset(chi_check, 0, sizeof(double) * 4 * n);
  S3oOut O;
  if (n_lanes == 64) {
    HostLanes<64> L;
    s3o_visit(L, V, P, O);
  } else {
    HostLanes<1> L;
    s3o_visit(L, V, P, O);
  }
  memcpy(st_out, &O.st, sizeof(O.st));
  ints[0] = O.returned0 ? 0 : O.n_inliers, ints[1] = O.n_bad, ints[2] = O.returned0, ints[3] = O.n_trials;
  ints[4] = O.iterations[0], ints[5] = O.iterations[1], ints[6] = O.trials[0], ints[7] = O.trials[1];
}

}  // extern "C"
