// Stand-alone evaluator of the fast single-lane forms and the one-wavefront solver of k_pose_opt_vio
// (vieo_slam_amd/csrc/vio_fast_device.h), built and run by tests/test_vio_fast_algebra.py.  One __global__ kernel per
// family (R rotations, P the prior edge, I the inertial edge, N the retraction, V the visual edge, S the solver), one
// lane per case; the solver runs one case per 64-thread workgroup with H, b, x and the column buffers in LDS, named in
// the LDS address space as the kernel names them.  Beside every fast form the plain form of imu_device.h is evaluated
// on the same inputs.  Built with the library's flags and, as pose_opt_vio.hip, with fused multiply-adds allowed.
// Nothing is compared here: the program reads named arrays, evaluates, writes named arrays (the VIEOALG1 layout of
// device_algebra_test.hip).  Exit code 0 = every family ran; otherwise the family's name is on stderr and nothing was
// launched after the error.
//
//   vio_fast_test in.bin out.bin
#pragma clang fp contract(fast)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../vieo_slam_amd/csrc/vio_fast_device.h"

using namespace vieo;

// ---------------------------------------------------------------- files
struct Entry {
  char name[32];
  int32_t dtype, reserved;
  int64_t count, offset;
};
static_assert(sizeof(Entry) == 56, "table of contents entry");

static const char* g_family = "input";
[[noreturn]] static void die(const char* what, const char* detail) {
  fprintf(stderr, "vio_fast_test: family %s: %s: %s\n", g_family, what, detail);
  exit(3);
}
#define CK(x)                                             \
  do {                                                    \
    const hipError_t e_ = (x);                            \
    if (e_ != hipSuccess) die(#x, hipGetErrorString(e_)); \
  } while (0)

struct Blob {
  std::vector<char> bytes;
  std::vector<Entry> toc;
  void load(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) die("open", path);
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    bytes.resize(n);
    if (n < 16 || fread(bytes.data(), 1, n, f) != (size_t)n) die("read", path);
    fclose(f);
    if (memcmp(bytes.data(), "VIEOALG1", 8)) die("magic", path);
    int32_t ne;
    memcpy(&ne, bytes.data() + 8, 4);
    if (ne < 0 || 16 + (int64_t)ne * (int64_t)sizeof(Entry) > n) die("table of contents", path);
    toc.resize(ne);
    memcpy(toc.data(), bytes.data() + 16, ne * sizeof(Entry));
    for (const Entry& e : toc) {
      const int64_t sz = e.dtype == 0 ? 8 : 4;
      if (e.count < 0 || e.offset < 0 || e.offset + e.count * sz > n) die("entry out of the file", e.name);
    }
  }
  const void* find(const char* name, int dtype, int64_t* count) const {
    for (const Entry& e : toc)
      if (!strncmp(e.name, name, 32)) {
        if (e.dtype != dtype) die("dtype of", name);
        *count = e.count;
        return bytes.data() + e.offset;
      }
    die("missing array", name);
  }
};

struct Out {
  std::vector<Entry> toc;
  std::vector<std::vector<char>> data;
  void add(const char* name, int dtype, const void* p, int64_t count) {
    Entry e;
    memset(&e, 0, sizeof(e));
    strncpy(e.name, name, 31);
    e.dtype = dtype, e.count = count;
    toc.push_back(e);
    const size_t sz = (size_t)count * (dtype == 0 ? 8 : 4);
    data.emplace_back((const char*)p, (const char*)p + sz);
  }
  void write(const char* path) {
    int64_t off = 16 + (int64_t)toc.size() * (int64_t)sizeof(Entry);
    for (size_t i = 0; i < toc.size(); i++) toc[i].offset = off, off += (int64_t)data[i].size();
    FILE* f = fopen(path, "wb");
    if (!f) die("open", path);
    const int32_t hdr[2] = {(int32_t)toc.size(), 0};
    bool ok = fwrite("VIEOALG1", 1, 8, f) == 8 && fwrite(hdr, 4, 2, f) == 2;
    ok = ok && (toc.empty() || fwrite(toc.data(), sizeof(Entry), toc.size(), f) == toc.size());
    for (const auto& d : data) ok = ok && (d.empty() || fwrite(d.data(), 1, d.size(), f) == d.size());
    if (fclose(f) || !ok) die("write", path);
  }
};

static Blob g_in;
static Out g_out;
static const int kMaxCases = 4096;

template <class T>
static const T* dev_in(const char* name, int per, int* n) {
  int64_t count;
  const void* h = g_in.find(name, sizeof(T) == 8 ? 0 : 1, &count);
  if (count % per) die("row length of", name);
  *n = (int)(count / per);
  if (*n > kMaxCases) die("more than 4096 cases in", name);
  T* d = nullptr;
  CK(hipMalloc(&d, (size_t)(count ? count : 1) * sizeof(T)));
  if (count) CK(hipMemcpy(d, h, (size_t)count * sizeof(T), hipMemcpyHostToDevice));
  return d;
}
static void same_n(const char* name, int a, int b) {
  if (a != b) die("case count of", name);
}
struct DevOut {
  const char* name;
  double* d;
  int64_t count;
};
static std::vector<DevOut> g_pending;
static double* dev_out(const char* name, int64_t count) {
  double* d = nullptr;
  CK(hipMalloc(&d, (size_t)(count ? count : 1) * 8));
  CK(hipMemset(d, 0, (size_t)(count ? count : 1) * 8));
  g_pending.push_back({name, d, count});
  return d;
}
static void finish_family() {
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  for (const DevOut& o : g_pending) {
    std::vector<double> h((size_t)o.count);
    if (o.count) CK(hipMemcpy(h.data(), o.d, (size_t)o.count * 8, hipMemcpyDeviceToHost));
    g_out.add(o.name, 0, h.data(), o.count);
  }
  g_pending.clear();
}
static inline int blocks_of(int n) { return n > 0 ? (n + 63) / 64 : 1; }

// a state is (p[3], v[3], qw, qx, qy, qz, bg[3], ba[3], dbg[3], dba[3])
__device__ static void load_state(const double* e, NSd& s) {
  for (int k = 0; k < 3; k++)
    s.p[k] = e[k], s.v[k] = e[3 + k], s.bg[k] = e[10 + k], s.ba[k] = e[13 + k], s.dbg[k] = e[16 + k], s.dba[k] = e[19 + k];
  s.qw = e[6], s.qx = e[7], s.qy = e[8], s.qz = e[9];
}
__device__ static void store_state(const NSd& s, double* o) {
  for (int k = 0; k < 3; k++)
    o[k] = s.p[k], o[3 + k] = s.v[k], o[10 + k] = s.bg[k], o[13 + k] = s.ba[k], o[16 + k] = s.dbg[k], o[19 + k] = s.dba[k];
  o[6] = s.qw, o[7] = s.qx, o[8] = s.qy, o[9] = s.qz;
}
__device__ static void put_q(double* o, const Qd& q) { o[0] = q.w, o[1] = q.x, o[2] = q.y, o[3] = q.z; }

// ---------------------------------------------------------------- R. rotations
// per rotation vector: so3_exp_unit (q, ok), so3_exp_q, so3_Jr_unit, so3_Jr_d
// per quaternion: q_renorm (q, ok), q_norm; so3_log_unit on the quaternion as given (log, g, ok) and behind q_renorm
// (log, g, ok); so3_log_q of the quaternion as given and behind q_norm; so3_JrInv_g of (log, g), so3_JrInv_d of the plain
// log; so3_JrInv_g_of and its inlined twin on the plain log
// per number: rcp_nr
__global__ void k_rotations(int n_w, const double* w, int n_q, const double* q, int n_d, const double* d, double* o_exp,
                            double* o_exp_p, double* o_jr, double* o_jr_p, double* o_ren, double* o_norm, double* o_log,
                            double* o_logc, double* o_log_p, double* o_logc_p, double* o_jri, double* o_jri_p, double* o_gof,
                            double* o_rcp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_w) {
    const double v[3] = {w[i * 3], w[i * 3 + 1], w[i * 3 + 2]};
    bool ok = true;
    put_q(o_exp + i * 5, so3_exp_unit(v, ok));
    o_exp[i * 5 + 4] = ok ? 1.0 : 0.0;
    put_q(o_exp_p + i * 4, so3_exp_q(v));
    double J[9];
    so3_Jr_unit(v, J);
    for (int k = 0; k < 9; k++) o_jr[i * 9 + k] = J[k];
    so3_Jr_d(v, J);
    for (int k = 0; k < 9; k++) o_jr_p[i * 9 + k] = J[k];
  }
  if (i < n_q) {
    const Qd a = Qd{q[i * 4], q[i * 4 + 1], q[i * 4 + 2], q[i * 4 + 3]};
    bool ok = true;
    const Qd r = q_renorm(a, ok);
    put_q(o_ren + i * 5, r);
    o_ren[i * 5 + 4] = ok ? 1.0 : 0.0;
    put_q(o_norm + i * 4, q_norm(a));
    double l[3], g, J[9];
    so3_log_unit(r, l, &g, ok);  // behind q_renorm, ok carried on
    for (int k = 0; k < 3; k++) o_logc[i * 5 + k] = l[k];
    o_logc[i * 5 + 3] = g, o_logc[i * 5 + 4] = ok ? 1.0 : 0.0;
    ok = true;
    so3_log_unit(a, l, &g, ok);
    for (int k = 0; k < 3; k++) o_log[i * 5 + k] = l[k];
    o_log[i * 5 + 3] = g, o_log[i * 5 + 4] = ok ? 1.0 : 0.0;
    so3_JrInv_g(l, g, J);
    for (int k = 0; k < 9; k++) o_jri[i * 9 + k] = J[k];
    double lp[3];
    so3_log_q(q_norm(a), lp);
    for (int k = 0; k < 3; k++) o_logc_p[i * 3 + k] = lp[k];
    so3_log_q(a, lp);
    for (int k = 0; k < 3; k++) o_log_p[i * 3 + k] = lp[k];
    so3_JrInv_d(lp, J);
    for (int k = 0; k < 9; k++) o_jri_p[i * 9 + k] = J[k];
    o_gof[i * 2] = so3_JrInv_g_of(lp), o_gof[i * 2 + 1] = so3_JrInv_g_of_inl(lp);
  }
  if (i < n_d) o_rcp[i] = rcp_nr(d[i]);
}

static void run_rotations() {
  g_family = "R.rotations";
  int n_w, n_q, n_d;
  const double* w = dev_in<double>("R.rotvec", 3, &n_w);
  const double* q = dev_in<double>("R.quat", 4, &n_q);
  const double* d = dev_in<double>("R.rcp_in", 1, &n_d);
  double* o_exp = dev_out("R.so3_exp_unit", n_w * 5);
  double* o_exp_p = dev_out("R.so3_exp_q", n_w * 4);
  double* o_jr = dev_out("R.so3_Jr_unit", n_w * 9);
  double* o_jr_p = dev_out("R.so3_Jr_d", n_w * 9);
  double* o_ren = dev_out("R.q_renorm", n_q * 5);
  double* o_norm = dev_out("R.q_norm", n_q * 4);
  double* o_log = dev_out("R.so3_log_unit", n_q * 5);
  double* o_logc = dev_out("R.so3_log_unit.renorm", n_q * 5);
  double* o_log_p = dev_out("R.so3_log_q", n_q * 3);
  double* o_logc_p = dev_out("R.so3_log_q.norm", n_q * 3);
  double* o_jri = dev_out("R.so3_JrInv_g", n_q * 9);
  double* o_jri_p = dev_out("R.so3_JrInv_d", n_q * 9);
  double* o_gof = dev_out("R.so3_JrInv_g_of", n_q * 2);
  double* o_rcp = dev_out("R.rcp_nr", n_d);
  int n = n_w;
  for (int v : {n_q, n_d}) n = v > n ? v : n;
  hipLaunchKernelGGL(k_rotations, dim3(blocks_of(n)), dim3(64), 0, 0, n_w, w, n_q, q, n_d, d, o_exp, o_exp_p, o_jr, o_jr_p,
                     o_ren, o_norm, o_log, o_logc, o_log_p, o_logc_p, o_jri, o_jri_p, o_gof, o_rcp);
  finish_family();
}

// ---------------------------------------------------------------- P. the prior edge
// per case (prior state, state i): for LEAF = false and true: err[15], the cache (qp[4], g_p), and the 15 x 15 Jacobian
// that prior_jacobian_init and prior_linearize leave in a buffer of NaN; the chain's ok; the plain forms' rotation rows,
// so3_JrInv_d of them and so3_JrInv_g_of
// (each form under test, the chain that yields ok and the plain forms are functions of their own, out of line: inlined
// into one kernel they would share common subexpressions, and with them the compiler's choice of what to fuse)
template <bool LEAF>
__device__ __noinline__ static void prior_one(const NSd& pr, const NSd& si, double* o_err, double* o_cache, double* o_J) {
  RotCache C;
  double err[15], J[225];
  prior_error<LEAF>(pr, si, err, C);
  for (int k = 0; k < 15; k++) o_err[k] = err[k];
  put_q(o_cache, C.qp);
  o_cache[4] = C.g_p;
  for (int k = 0; k < 225; k++) J[k] = __builtin_nan("");
  prior_jacobian_init(J, 0, 1);
  prior_linearize(err, J, C);
  for (int k = 0; k < 225; k++) o_J[k] = J[k];
}
__device__ __noinline__ static void prior_ok(const NSd& pr, const NSd& si, double* o_ok) {
  bool ok = true;
  const Qd q = q_renorm(q_mul(q_conj(q_of(pr)), q_of(si)), ok);
  double l[3], g;
  so3_log_unit(q, l, &g, ok);
  *o_ok = ok ? 1.0 : 0.0;
}
__device__ __noinline__ static void prior_plain(const NSd& pr, const NSd& si, double* o) {
  const Qd qn = q_norm(q_mul(q_conj(q_of(pr)), q_of(si)));
  double l[3], J[9];
  so3_log_q(qn, l);
  so3_JrInv_d(l, J);
  put_q(o, qn);
  for (int k = 0; k < 3; k++) o[4 + k] = l[k];
  o[7] = so3_JrInv_g_of(l);
  for (int k = 0; k < 9; k++) o[8 + k] = J[k];
}
__global__ void k_prior(int n, const double* prs, const double* sis, double* o_err, double* o_cache, double* o_J,
                        double* o_errL, double* o_cacheL, double* o_JL, double* o_ok, double* o_plain) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  NSd pr, si;
  load_state(prs + i * 22, pr), load_state(sis + i * 22, si);
  prior_one<false>(pr, si, o_err + i * 15, o_cache + i * 5, o_J + i * 225);
  prior_one<true>(pr, si, o_errL + i * 15, o_cacheL + i * 5, o_JL + i * 225);
  prior_ok(pr, si, o_ok + i);
  prior_plain(pr, si, o_plain + i * 17);
}

static void run_prior() {
  g_family = "P.prior";
  int n, m;
  const double* pr = dev_in<double>("P.prior", 22, &n);
  const double* si = dev_in<double>("P.state", 22, &m);
  same_n("P.state", n, m);
  double* o_err = dev_out("P.prior_error", n * 15);
  double* o_cache = dev_out("P.cache", n * 5);
  double* o_J = dev_out("P.prior_jacobian", (int64_t)n * 225);
  double* o_errL = dev_out("P.prior_error<LEAF>", n * 15);
  double* o_cacheL = dev_out("P.cache<LEAF>", n * 5);
  double* o_JL = dev_out("P.prior_jacobian<LEAF>", (int64_t)n * 225);
  double* o_ok = dev_out("P.ok", n);
  double* o_plain = dev_out("P.plain", n * 17);
  hipLaunchKernelGGL(k_prior, dim3(blocks_of(n)), dim3(64), 0, 0, n, pr, si, o_err, o_cache, o_J, o_errL, o_cacheL, o_JL, o_ok,
                     o_plain);
  finish_family();
}

// ---------------------------------------------------------------- I. the inertial edge
// a measurement is the first 61 doubles of vieo_imu_preint: dt, Rij, vij, pij, JgR, Jgv, Jav, Jgp, Jap.
// per case, for LEAF = false and true: err[9] (imu_error part 1 and imu_error_rot), the cache (qe[4], qb[4], g_e, w[3],
// w_small: 13), the Jacobian of imu_jacobian_init + imu_linearize_pv + imu_linearize_rot in a buffer of NaN (216);
// once: the Jacobian of imu_linearize part 1 + imu_linearize_rot in a cleared buffer, the chain's (ok, w_small), and the
// plain forms: imu_error and imu_linearize part 0, the quaternions qe and qb of the plain chain, so3_JrInv_g_of
template <bool LEAF>
__device__ __noinline__ static void imu_one(const vieo_imu_preint& M, const double* g, const NSd& a, const NSd& b, double* o_err,
                               double* o_cache, double* o_J, double* o_J1) {
  const Qd qRij = R_to_q(M.Rij);
  RotCache C;
  double err[9], J[216];
  for (int k = 0; k < 9; k++) err[k] = 0;
  imu_error(M, g, a, b, err, 6, 1);
  imu_error_rot<LEAF>(M, qRij, a, b, err, C);
  for (int k = 0; k < 9; k++) o_err[k] = err[k];
  put_q(o_cache, C.qe), put_q(o_cache + 4, C.qb);
  o_cache[8] = C.g_e, o_cache[9] = C.w[0], o_cache[10] = C.w[1], o_cache[11] = C.w[2], o_cache[12] = C.w_small;
  for (int k = 0; k < 216; k++) J[k] = __builtin_nan("");
  imu_jacobian_init(M, J, 0, 1);
  imu_linearize_pv(M, g, a, b, J);
  imu_linearize_rot(M, err, J, C);
  for (int k = 0; k < 216; k++) o_J[k] = J[k];
  if (o_J1) {
    for (int k = 0; k < 216; k++) J[k] = 0;
    imu_linearize(M, g, a, b, err, J, 6, 3, 1);
    imu_linearize_rot(M, err, J, C);
    for (int k = 0; k < 216; k++) o_J1[k] = J[k];
  }
}
__device__ __noinline__ static void imu_ok(const vieo_imu_preint& M, const NSd& a, const NSd& b, double* o_ok) {
  const Qd qRij = R_to_q(M.Rij);
  double w[3], l[3], gg;
  mv3(M.JgR, a.dbg, w);
  bool ok = true;
  const Qd qx = so3_exp_unit(w, ok);
  const bool w_small = ok;
  const Qd qb = q_renorm(q_mul(q_conj(q_of(a)), q_of(b)), ok);
  const Qd qa = q_renorm(q_mul(qRij, qx), ok);
  const Qd qe = q_renorm(q_mul(q_conj(qa), qb), ok);
  so3_log_unit(qe, l, &gg, ok);
  o_ok[0] = ok ? 1.0 : 0.0, o_ok[1] = w_small ? 1.0 : 0.0;
}
// the plain forms: imu_error and imu_linearize of imu_device.h (part 0), and the chain's quaternions (qe, qb) with
// so3_JrInv_g_of, which imu_error does not hand out
__device__ __noinline__ static void imu_plain(const vieo_imu_preint& M, const double* g, const NSd& a, const NSd& b,
                                              double* o_perr, double* o_pJ, double* o_pq) {
  double err[9], J[216];
  for (int k = 0; k < 9; k++) err[k] = 0;
  imu_error(M, g, a, b, err, 6, 0);
  for (int k = 0; k < 9; k++) o_perr[k] = err[k];
  imu_linearize(M, g, a, b, err, J, 6, 3, 0);
  for (int k = 0; k < 216; k++) o_pJ[k] = J[k];
  double w[3], l[3];
  mv3(M.JgR, a.dbg, w);
  const Qd pa = q_norm(q_mul(R_to_q(M.Rij), so3_exp_q(w)));
  const Qd pb = q_norm(q_mul(q_conj(q_of(a)), q_of(b)));
  const Qd pe = q_norm(q_mul(q_conj(pa), pb));
  put_q(o_pq, pe), put_q(o_pq + 4, pb);
  so3_log_q(pe, l);
  o_pq[8] = so3_JrInv_g_of(l);
}
__global__ void k_inertial(int n, const double* meas, const double* gw, const double* sis, const double* sjs, double* o_err,
                           double* o_cache, double* o_J, double* o_errL, double* o_cacheL, double* o_JL, double* o_J1,
                           double* o_ok, double* o_perr, double* o_pJ, double* o_pq) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  vieo_imu_preint M;
  {
    double* m = (double*)&M;
    for (int k = 0; k < 61; k++) m[k] = meas[i * 61 + k];
    for (int k = 0; k < 81; k++) M.Sigma[k] = 0;
  }
  const double g[3] = {gw[i * 3], gw[i * 3 + 1], gw[i * 3 + 2]};
  NSd a, b;
  load_state(sis + i * 22, a), load_state(sjs + i * 22, b);
  imu_one<false>(M, g, a, b, o_err + i * 9, o_cache + i * 13, o_J + (size_t)i * 216, o_J1 + (size_t)i * 216);
  imu_one<true>(M, g, a, b, o_errL + i * 9, o_cacheL + i * 13, o_JL + (size_t)i * 216, nullptr);
  imu_ok(M, a, b, o_ok + i * 2);
  imu_plain(M, g, a, b, o_perr + i * 9, o_pJ + (size_t)i * 216, o_pq + i * 9);
}

static void run_inertial() {
  g_family = "I.inertial";
  int n, m;
  const double* meas = dev_in<double>("I.meas", 61, &n);
  const double* gw = dev_in<double>("I.gw", 3, &m);
  same_n("I.gw", n, m);
  const double* si = dev_in<double>("I.si", 22, &m);
  same_n("I.si", n, m);
  const double* sj = dev_in<double>("I.sj", 22, &m);
  same_n("I.sj", n, m);
  double* o_err = dev_out("I.imu_error_rot", n * 9);
  double* o_cache = dev_out("I.cache", n * 13);
  double* o_J = dev_out("I.jacobian", (int64_t)n * 216);
  double* o_errL = dev_out("I.imu_error_rot<LEAF>", n * 9);
  double* o_cacheL = dev_out("I.cache<LEAF>", n * 13);
  double* o_JL = dev_out("I.jacobian<LEAF>", (int64_t)n * 216);
  double* o_J1 = dev_out("I.jacobian.part1", (int64_t)n * 216);
  double* o_ok = dev_out("I.ok", n * 2);
  double* o_perr = dev_out("I.imu_error", n * 9);
  double* o_pJ = dev_out("I.imu_linearize", (int64_t)n * 216);
  double* o_pq = dev_out("I.plain", n * 9);
  hipLaunchKernelGGL(k_inertial, dim3(blocks_of(n)), dim3(64), 0, 0, n, meas, gw, si, sj, o_err, o_cache, o_J, o_errL, o_cacheL,
                     o_JL, o_J1, o_ok, o_perr, o_pJ, o_pq);
  finish_family();
}

// ---------------------------------------------------------------- N. the retraction
// per case: ns_inc_unit once (state, ok of its chain), ns_inc once, and ns_inc_unit `reps` times in a row
__global__ void k_retraction(int n, const double* ss, const double* d9, const double* db6, int reps, double* o_fast,
                             double* o_ok, double* o_plain, double* o_rep) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  NSd s;
  double d[9], db[6];
  for (int k = 0; k < 9; k++) d[k] = d9[i * 9 + k];
  for (int k = 0; k < 6; k++) db[k] = db6[i * 6 + k];
  load_state(ss + i * 22, s);
  bool ok = true;
  (void)q_renorm(q_mul(q_of(s), so3_exp_unit(d + 6, ok)), ok);
  o_ok[i] = ok ? 1.0 : 0.0;
  ns_inc_unit(s, d, db);
  store_state(s, o_fast + i * 22);
  for (int r = 1; r < reps; r++) ns_inc_unit(s, d, db);
  store_state(s, o_rep + i * 22);
  load_state(ss + i * 22, s);
  ns_inc(s, d, db);
  store_state(s, o_plain + i * 22);
}

static void run_retraction() {
  g_family = "N.retraction";
  int n, m;
  const double* s = dev_in<double>("N.state", 22, &n);
  const double* d9 = dev_in<double>("N.state_inc", 9, &m);
  same_n("N.state_inc", n, m);
  const double* db = dev_in<double>("N.bias_inc", 6, &m);
  same_n("N.bias_inc", n, m);
  int64_t c;
  const int32_t* reps = (const int32_t*)g_in.find("N.reps", 1, &c);
  if (c != 1 || reps[0] < 1 || reps[0] > 100000) die("1 .. 100000 in", "N.reps");
  double* o_fast = dev_out("N.ns_inc_unit", n * 22);
  double* o_ok = dev_out("N.ok", n);
  double* o_plain = dev_out("N.ns_inc", n * 22);
  double* o_rep = dev_out("N.ns_inc_unit.repeated", n * 22);
  hipLaunchKernelGGL(k_retraction, dim3(blocks_of(n)), dim3(64), 0, 0, n, s, d9, db, reps[0], o_fast, o_ok, o_plain, o_rep);
  finish_family();
}

// ---------------------------------------------------------------- V. the visual edge
// a camera is (fx, fy, cx, cy, bf, Rcb[9], tcb[3]) -- the pinhole members the flat forms read.
// per slot: camera, pose (p, q), observation (Xw, u, v, ur, inv_sigma2: float values), (valid, robust), the Huber width
// and the 27 sums before.  Outputs: (err[3], Pc[3], info, chi2, stereo: 9) of vis_error_flat, (rho, rho') of huber_flat
// at that chi2, J[18] of vis_jacobian_flat, the 27 sums after vis_accumulate_flat with the slot's weight (info of a
// valid slot, 0 otherwise) -- and beside them edge_error / huber / visual_jacobian / visual_accumulate of ba_device.h.
__global__ void k_visual(const CamD* cams, int n, const int* cam, const double* est, const double* obsf, const int* vr,
                         const double* delta, const double* acc0, double* o_e, double* o_h, double* o_j, double* o_acc,
                         double* o_pe, double* o_ph, double* o_pj, double* o_pacc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const CamD& c = cams[cam[i]];
  Est s;
  const double* e = est + i * 7;
  s.p[0] = e[0], s.p[1] = e[1], s.p[2] = e[2], s.qw = e[3], s.qx = e[4], s.qy = e[5], s.qz = e[6];
  vieo_pose_obs o;
  const double* f = obsf + i * 7;
  o.Xw[0] = (float)f[0], o.Xw[1] = (float)f[1], o.Xw[2] = (float)f[2];
  o.u = (float)f[3], o.v = (float)f[4], o.ur = (float)f[5], o.inv_sigma2 = (float)f[6], o.flags = 1;
  const bool valid = vr[i * 2] != 0, robust = vr[i * 2 + 1] != 0;
  PoseXf X;
  make_xf(c, s, X);
  VisFlat E;
  vis_error_flat(c, X, o, valid, E);
  for (int k = 0; k < 3; k++) o_e[i * 9 + k] = E.err[k], o_e[i * 9 + 3 + k] = E.Pc[k];
  o_e[i * 9 + 6] = E.info, o_e[i * 9 + 7] = E.chi2, o_e[i * 9 + 8] = E.stereo ? 1.0 : 0.0;
  const double d = delta[i];
  double r0, r1, J[18], acc[27];
  huber_flat(E.chi2, d, d * d, robust, &r0, &r1);
  o_h[i * 2] = r0, o_h[i * 2 + 1] = r1;
  vis_jacobian_flat(c, X, s.p, o, E, J);
  for (int k = 0; k < 18; k++) o_j[i * 18 + k] = J[k];
  for (int k = 0; k < 27; k++) acc[k] = acc0[i * 27 + k];
  vis_accumulate_flat(J, E.err, valid ? E.info : 0.0, r1, acc);
  for (int k = 0; k < 27; k++) o_acc[i * 27 + k] = acc[k];
  if (!valid) return;  // the plain forms divide by the depth
  double err[3], Pc[3];
  const double chi2 = edge_error(c, X, o, err, Pc);
  o_pe[i * 7] = chi2;
  for (int k = 0; k < 3; k++) o_pe[i * 7 + 1 + k] = err[k], o_pe[i * 7 + 4 + k] = Pc[k];
  huber(chi2, d, d * d, &r0, &r1);
  o_ph[i * 2] = r0, o_ph[i * 2 + 1] = r1;
  for (int k = 0; k < 18; k++) J[k] = 0;
  visual_jacobian(c, X, s.p, o, Pc, J);
  for (int k = 0; k < 18; k++) o_pj[i * 18 + k] = J[k];
  for (int k = 0; k < 27; k++) acc[k] = acc0[i * 27 + k];
  visual_accumulate(J, err, (double)o.inv_sigma2, r1, o.ur >= 0, acc);
  for (int k = 0; k < 27; k++) o_pacc[i * 27 + k] = acc[k];
}

__global__ void k_huber(int n, const double* e, const double* delta, const double* dsqr, const int* robust, double* o,
                        double* o_p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double r0, r1;
  huber_flat(e[i], delta[i], dsqr[i], robust[i] != 0, &r0, &r1);
  o[i * 2] = r0, o[i * 2 + 1] = r1;
  huber(e[i], delta[i], dsqr[i], &r0, &r1);
  o_p[i * 2] = r0, o_p[i * 2 + 1] = r1;
}

static void run_visual() {
  g_family = "V.visual_edge";
  int64_t cf;
  const double* hf = (const double*)g_in.find("V.cam_f64", 0, &cf);
  if (cf % 17 || cf / 17 < 1 || cf / 17 > 64) die("camera table", "V.cam_f64");
  const int n_cams = (int)(cf / 17);
  std::vector<CamD> hc(n_cams);
  for (int c = 0; c < n_cams; c++) {
    const double* f = hf + c * 17;
    CamD& d = hc[c];
    memset(&d, 0, sizeof(d));
    d.fx = f[0], d.fy = f[1], d.cx = f[2], d.cy = f[3], d.bf = f[4];
    for (int k = 0; k < 9; k++) d.Rcb[k] = f[5 + k];
    for (int k = 0; k < 3; k++) d.tcb[k] = f[14 + k];
    d.model = 0, d.num_k = 0;
  }
  CamD* cams = nullptr;
  CK(hipMalloc(&cams, hc.size() * sizeof(CamD)));
  CK(hipMemcpy(cams, hc.data(), hc.size() * sizeof(CamD), hipMemcpyHostToDevice));
  int n, m;
  const int* cam = dev_in<int>("V.cam", 1, &n);
  {
    int64_t c;
    const int32_t* h = (const int32_t*)g_in.find("V.cam", 1, &c);
    for (int i = 0; i < n; i++)
      if (h[i] < 0 || h[i] >= n_cams) die("camera index out of range in", "V.cam");
  }
  const double* est = dev_in<double>("V.pose", 7, &m);
  same_n("V.pose", n, m);
  const double* obs = dev_in<double>("V.obs", 7, &m);
  same_n("V.obs", n, m);
  const int* vr = dev_in<int>("V.valid_robust", 2, &m);
  same_n("V.valid_robust", n, m);
  const double* delta = dev_in<double>("V.delta", 1, &m);
  same_n("V.delta", n, m);
  const double* acc0 = dev_in<double>("V.acc0", 27, &m);
  same_n("V.acc0", n, m);
  double* o_e = dev_out("V.vis_error_flat", n * 9);
  double* o_h = dev_out("V.edge_huber_flat", n * 2);
  double* o_j = dev_out("V.vis_jacobian_flat", n * 18);
  double* o_acc = dev_out("V.vis_accumulate_flat", n * 27);
  double* o_pe = dev_out("V.edge_error", n * 7);
  double* o_ph = dev_out("V.edge_huber", n * 2);
  double* o_pj = dev_out("V.visual_jacobian", n * 18);
  double* o_pacc = dev_out("V.visual_accumulate", n * 27);
  hipLaunchKernelGGL(k_visual, dim3(blocks_of(n)), dim3(64), 0, 0, cams, n, cam, est, obs, vr, delta, acc0, o_e, o_h, o_j,
                     o_acc, o_pe, o_ph, o_pj, o_pacc);
  finish_family();
  g_family = "V.huber";
  const double* he = dev_in<double>("V.huber_e", 1, &n);
  const double* hd = dev_in<double>("V.huber_delta", 1, &m);
  same_n("V.huber_delta", n, m);
  const double* hq = dev_in<double>("V.huber_dsqr", 1, &m);
  same_n("V.huber_dsqr", n, m);
  const int* hr = dev_in<int>("V.huber_robust", 1, &m);
  same_n("V.huber_robust", n, m);
  double* ho = dev_out("V.huber_flat", n * 2);
  double* hp = dev_out("V.huber", n * 2);
  hipLaunchKernelGGL(k_huber, dim3(blocks_of(n)), dim3(64), 0, 0, n, he, hd, hq, hr, ho, hp);
  finish_family();
}

// ---------------------------------------------------------------- S. the solver
// one case per 64-thread workgroup: n (15 or 30), H (n x n row-major in the first n * n of 900 doubles), b[32], lambda
// and what x holds before the call.  H, b, x and the column buffers are __shared__ arrays handed over as lds_f64*, the
// way k_pose_opt_vio hands S.H, S.b, S.x and S.L; the column buffers start as NaN.  Outputs: x[32] and the return value.
__global__ void __launch_bounds__(64) k_solve(const int* ns, const double* Hg, const double* bg, const double* lam,
                                              const double* x0, double* xo, double* ret) {
  __shared__ double H[900], L[900], b[32], x[32];
  const int c = blockIdx.x, lane = threadIdx.x, n = ns[c];
  for (int i = lane; i < 900; i += 64) H[i] = Hg[(size_t)c * 900 + i], L[i] = __builtin_nan("");
  if (lane < 32) b[lane] = bg[c * 32 + lane], x[lane] = x0[c * 32 + lane];
  __syncthreads();
  const double lambda = lam[c];
  const bool ok = n == 15 ? wave_solve_vio<9>((const lds_f64*)H, n, lambda, (const lds_f64*)b, (lds_f64*)x, (lds_f64*)L, lane)
                          : wave_solve_vio<24>((const lds_f64*)H, n, lambda, (const lds_f64*)b, (lds_f64*)x, (lds_f64*)L, lane);
  __syncthreads();
  if (lane < 32) xo[c * 32 + lane] = x[lane];
  if (lane == 0) ret[c] = ok ? 1.0 : 0.0;
}

static void run_solver() {
  g_family = "S.solver";
  int n, m;
  const int* ns = dev_in<int>("S.n", 1, &n);
  {
    int64_t c;
    const int32_t* h = (const int32_t*)g_in.find("S.n", 1, &c);
    for (int i = 0; i < n; i++)
      if (h[i] != 15 && h[i] != 30) die("n is 15 or 30 in", "S.n");
  }
  const double* H = dev_in<double>("S.H", 900, &m);
  same_n("S.H", n, m);
  const double* b = dev_in<double>("S.b", 32, &m);
  same_n("S.b", n, m);
  const double* lam = dev_in<double>("S.lambda", 1, &m);
  same_n("S.lambda", n, m);
  const double* x0 = dev_in<double>("S.x0", 32, &m);
  same_n("S.x0", n, m);
  double* xo = dev_out("S.x", n * 32);
  double* ret = dev_out("S.ok", n);
  if (n > 0) hipLaunchKernelGGL(k_solve, dim3(n), dim3(64), 0, 0, ns, H, b, lam, x0, xo, ret);
  finish_family();
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
    return 2;
  }
  g_in.load(argv[1]);
  run_rotations();
  run_prior();
  run_inertial();
  run_retraction();
  run_visual();
  run_solver();
  g_family = "output";
  g_out.write(argv[2]);
  return 0;
}
