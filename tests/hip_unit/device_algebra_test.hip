// Stand-alone evaluator of the lane functions the optimisers are assembled from (built and run by
// tests/test_device_algebra.py): ba_device.h, imu_device.h, cam_project.h, cam_unproject.h, triangulate.h.  One __global__ kernel per
// family (A rotations, B retractions, C cameras, D the visual edge, E the inertial and encoder edges, F triangulation)
// with one lane per case; the reductions (G) launch the real workgroup shapes.  Built with the library's flags,
// VIEO_POSE_DPP64 undefined.
// Nothing is compared here: the program reads named arrays, evaluates, writes named arrays, and the test compares them
// with a 50-digit reference.
//
//   device_algebra_test in.bin out.bin
//
// File layout (little endian), the same for both files:
//   char magic[8] = "VIEOALG1"; int32 n_entries; int32 reserved;
//   n_entries x { char name[32]; int32 dtype (0 = f64, 1 = i32); int32 reserved; int64 count; int64 byte_offset; }
//   the arrays, each at its byte_offset from the start of the file.
// Exit code 0 = every family ran; otherwise the family's name is on stderr and nothing was launched after the error.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../vieo_slam_amd/csrc/ba_device.h"
#include "../../vieo_slam_amd/csrc/cam_project.h"
#include "../../vieo_slam_amd/csrc/cam_unproject.h"
#include "../../vieo_slam_amd/csrc/imu_device.h"
#include "../../vieo_slam_amd/csrc/triangulate.h"

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
  fprintf(stderr, "device_algebra_test: family %s: %s: %s\n", g_family, what, detail);
  exit(3);
}
#define CK(x)                                         \
  do {                                                \
    const hipError_t e_ = (x);                        \
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

// input array `name` (count = n * per) on the device; n comes back
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
// the family's kernel is launched: wait for it, then fetch what it wrote
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

// ---------------------------------------------------------------- A. rotations
__global__ void k_rotations(int n_w, const double* w, int n_q, const double* q, int n_r, const double* R, int n_m,
                            const double* qa, const double* qb, int n_n, const double* qr, double* o_exp, double* o_jr,
                            double* o_jrinv, double* o_log, double* o_q2r, double* o_r2q, double* o_mul, double* o_norm) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_w) {
    const double v[3] = {w[i * 3], w[i * 3 + 1], w[i * 3 + 2]};
    const Qd e = so3_exp_q(v);
    o_exp[i * 4] = e.w, o_exp[i * 4 + 1] = e.x, o_exp[i * 4 + 2] = e.y, o_exp[i * 4 + 3] = e.z;
    double J[9];
    so3_Jr_d(v, J);
    for (int k = 0; k < 9; k++) o_jr[i * 9 + k] = J[k];
    so3_JrInv_d(v, J);
    for (int k = 0; k < 9; k++) o_jrinv[i * 9 + k] = J[k];
  }
  if (i < n_q) {
    const Qd a = Qd{q[i * 4], q[i * 4 + 1], q[i * 4 + 2], q[i * 4 + 3]};
    double l[3], M[9];
    so3_log_q(a, l);
    for (int k = 0; k < 3; k++) o_log[i * 3 + k] = l[k];
    Est e;
    e.p[0] = e.p[1] = e.p[2] = 0;
    e.qw = a.w, e.qx = a.x, e.qy = a.y, e.qz = a.z;
    quat_to_R(e, M);
    for (int k = 0; k < 9; k++) o_q2r[i * 9 + k] = M[k];
  }
  if (i < n_r) {
    double M[9];
    for (int k = 0; k < 9; k++) M[k] = R[i * 9 + k];
    const Qd a = R_to_q(M);
    o_r2q[i * 4] = a.w, o_r2q[i * 4 + 1] = a.x, o_r2q[i * 4 + 2] = a.y, o_r2q[i * 4 + 3] = a.z;
  }
  if (i < n_m) {
    const Qd a = Qd{qa[i * 4], qa[i * 4 + 1], qa[i * 4 + 2], qa[i * 4 + 3]};
    const Qd b = Qd{qb[i * 4], qb[i * 4 + 1], qb[i * 4 + 2], qb[i * 4 + 3]};
    const Qd c = q_mul(a, b);
    o_mul[i * 4] = c.w, o_mul[i * 4 + 1] = c.x, o_mul[i * 4 + 2] = c.y, o_mul[i * 4 + 3] = c.z;
  }
  if (i < n_n) {
    const Qd c = q_norm(Qd{qr[i * 4], qr[i * 4 + 1], qr[i * 4 + 2], qr[i * 4 + 3]});
    o_norm[i * 4] = c.w, o_norm[i * 4 + 1] = c.x, o_norm[i * 4 + 2] = c.y, o_norm[i * 4 + 3] = c.z;
  }
}

static void run_rotations() {
  g_family = "A.rotations";
  int n_w, n_q, n_r, n_m, n_m2, n_n;
  const double* w = dev_in<double>("A.rotvec", 3, &n_w);
  const double* q = dev_in<double>("A.quat", 4, &n_q);
  const double* R = dev_in<double>("A.mat", 9, &n_r);
  const double* qa = dev_in<double>("A.mul_a", 4, &n_m);
  const double* qb = dev_in<double>("A.mul_b", 4, &n_m2);
  same_n("A.mul_b", n_m, n_m2);
  const double* qr = dev_in<double>("A.raw_quat", 4, &n_n);
  double* o_exp = dev_out("A.so3_exp_q", n_w * 4);
  double* o_jr = dev_out("A.so3_Jr_d", n_w * 9);
  double* o_jrinv = dev_out("A.so3_JrInv_d", n_w * 9);
  double* o_log = dev_out("A.so3_log_q", n_q * 3);
  double* o_q2r = dev_out("A.quat_to_R", n_q * 9);
  double* o_r2q = dev_out("A.R_to_q", n_r * 4);
  double* o_mul = dev_out("A.q_mul", n_m * 4);
  double* o_norm = dev_out("A.q_norm", n_n * 4);
  int n = n_w;
  for (int v : {n_q, n_r, n_m, n_n}) n = v > n ? v : n;
  hipLaunchKernelGGL(k_rotations, dim3(blocks_of(n)), dim3(64), 0, 0, n_w, w, n_q, q, n_r, R, n_m, qa, qb, n_n, qr, o_exp,
                     o_jr, o_jrinv, o_log, o_q2r, o_r2q, o_mul, o_norm);
  finish_family();
}

// ---------------------------------------------------------------- B. retractions
// a pose is (p[3], qw, qx, qy, qz); a state is (p[3], v[3], qw, qx, qy, qz, bg[3], ba[3], dbg[3], dba[3])
__global__ void k_retractions(int n_pr, const double* est, const double* d6, double* o_pr, int n_ns, const double* ns,
                              const double* d9, const double* db6, double* o_ns) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_pr) {
    const double* e = est + i * 7;
    Est s;
    s.p[0] = e[0], s.p[1] = e[1], s.p[2] = e[2], s.qw = e[3], s.qx = e[4], s.qy = e[5], s.qz = e[6];
    double d[6];
    for (int k = 0; k < 6; k++) d[k] = d6[i * 6 + k];
    inc_small_pr(s, d);
    double* o = o_pr + i * 7;
    o[0] = s.p[0], o[1] = s.p[1], o[2] = s.p[2], o[3] = s.qw, o[4] = s.qx, o[5] = s.qy, o[6] = s.qz;
  }
  if (i < n_ns) {
    const double* e = ns + i * 22;
    NSd s;
    for (int k = 0; k < 3; k++)
      s.p[k] = e[k], s.v[k] = e[3 + k], s.bg[k] = e[10 + k], s.ba[k] = e[13 + k], s.dbg[k] = e[16 + k], s.dba[k] = e[19 + k];
    s.qw = e[6], s.qx = e[7], s.qy = e[8], s.qz = e[9];
    double d[9], db[6];
    for (int k = 0; k < 9; k++) d[k] = d9[i * 9 + k];
    for (int k = 0; k < 6; k++) db[k] = db6[i * 6 + k];
    ns_inc(s, d, db);
    double* o = o_ns + i * 22;
    for (int k = 0; k < 3; k++)
      o[k] = s.p[k], o[3 + k] = s.v[k], o[10 + k] = s.bg[k], o[13 + k] = s.ba[k], o[16 + k] = s.dbg[k], o[19 + k] = s.dba[k];
    o[6] = s.qw, o[7] = s.qx, o[8] = s.qy, o[9] = s.qz;
  }
}

static void run_retractions() {
  g_family = "B.retractions";
  int n_pr, n_ns, m;
  const double* est = dev_in<double>("B.pose", 7, &n_pr);
  const double* d6 = dev_in<double>("B.pose_inc", 6, &m);
  same_n("B.pose_inc", n_pr, m);
  const double* ns = dev_in<double>("B.state", 22, &n_ns);
  const double* d9 = dev_in<double>("B.state_inc", 9, &m);
  same_n("B.state_inc", n_ns, m);
  const double* db6 = dev_in<double>("B.bias_inc", 6, &m);
  same_n("B.bias_inc", n_ns, m);
  double* o_pr = dev_out("B.inc_small_pr", n_pr * 7);
  double* o_ns = dev_out("B.ns_inc", n_ns * 22);
  const int n = n_pr > n_ns ? n_pr : n_ns;
  hipLaunchKernelGGL(k_retractions, dim3(blocks_of(n)), dim3(64), 0, 0, n_pr, est, d6, o_pr, n_ns, ns, d9, db6, o_ns);
  finish_family();
}

// ---------------------------------------------------------------- C. cameras
__global__ void k_cameras(const CamD* cams, int n_p, const int* pc, const double* P, double* o_uvj, double* o_j,
                          double* o_uv, int n_u, const int* uc, const double* uvf, double* o_un, int n_h, const int* hc,
                          const double* uvd, double* o_pin) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_p) {
    const double X[3] = {P[i * 3], P[i * 3 + 1], P[i * 3 + 2]};
    double uv[2], J[6];
    cam_project(cams[pc[i]], X, uv, J);
    o_uvj[i * 2] = uv[0], o_uvj[i * 2 + 1] = uv[1];
    for (int k = 0; k < 6; k++) o_j[i * 6 + k] = J[k];
    cam_project(cams[pc[i]], X, uv, nullptr);
    o_uv[i * 2] = uv[0], o_uv[i * 2 + 1] = uv[1];
  }
  if (i < n_u) {
    double X[3];
    cam_unproject(cams[uc[i]], (float)uvf[i * 2], (float)uvf[i * 2 + 1], X);
    for (int k = 0; k < 3; k++) o_un[i * 3 + k] = X[k];
  }
  if (i < n_h) {
    double X[3];
    unproject_pinhole(cams[hc[i]], uvd[i * 2], uvd[i * 2 + 1], X);
    for (int k = 0; k < 3; k++) o_pin[i * 3 + k] = X[k];
  }
}

static void check_index(const char* name, int n, int n_cams) {
  int64_t c;
  const int32_t* h = (const int32_t*)g_in.find(name, 1, &c);
  for (int i = 0; i < n; i++)
    if (h[i] < 0 || h[i] >= n_cams) die("camera index out of range in", name);
}

static const CamD* upload_cameras(int* n_cams_out) {
  // a camera is (fx, fy, cx, cy, bf, Rcb[9], tcb[3], k[8]) in f64 and (model, num_k) in i32
  int64_t cf, ci;
  const double* hf = (const double*)g_in.find("C.cam_f64", 0, &cf);
  const int32_t* hi = (const int32_t*)g_in.find("C.cam_i32", 1, &ci);
  if (cf % 25 || ci % 2 || cf / 25 != ci / 2 || cf / 25 > 64) die("camera table", "C.cam_f64 / C.cam_i32");
  const int n_cams = (int)(cf / 25);
  std::vector<CamD> hc(n_cams ? n_cams : 1);
  for (int c = 0; c < n_cams; c++) {
    const double* f = hf + c * 25;
    CamD& d = hc[c];
    d.fx = f[0], d.fy = f[1], d.cx = f[2], d.cy = f[3], d.bf = f[4];
    for (int k = 0; k < 9; k++) d.Rcb[k] = f[5 + k];
    for (int k = 0; k < 3; k++) d.tcb[k] = f[14 + k];
    for (int k = 0; k < 8; k++) d.k[k] = f[17 + k];
    d.model = hi[c * 2], d.num_k = hi[c * 2 + 1];
    if (d.model < 0 || d.model > 2 || (d.model == 1 && (d.num_k < 2 || d.num_k > 6))) die("camera model", "C.cam_i32");
  }
  CamD* cams = nullptr;
  CK(hipMalloc(&cams, hc.size() * sizeof(CamD)));
  CK(hipMemcpy(cams, hc.data(), hc.size() * sizeof(CamD), hipMemcpyHostToDevice));
  *n_cams_out = n_cams;
  return cams;
}

static void run_cameras() {
  g_family = "C.cameras";
  int n_cams;
  const CamD* cams = upload_cameras(&n_cams);
  int n_p, n_u, n_h, m;
  const int* pc = dev_in<int>("C.project_cam", 1, &n_p);
  check_index("C.project_cam", n_p, n_cams);
  const double* P = dev_in<double>("C.project_P", 3, &m);
  same_n("C.project_P", n_p, m);
  const int* uc = dev_in<int>("C.unproject_cam", 1, &n_u);
  check_index("C.unproject_cam", n_u, n_cams);
  const double* uvf = dev_in<double>("C.unproject_uv", 2, &m);
  same_n("C.unproject_uv", n_u, m);
  const int* hcam = dev_in<int>("C.pinhole_cam", 1, &n_h);
  check_index("C.pinhole_cam", n_h, n_cams);
  const double* uvd = dev_in<double>("C.pinhole_uv", 2, &m);
  same_n("C.pinhole_uv", n_h, m);
  double* o_uvj = dev_out("C.cam_project.uv_with_J", n_p * 2);
  double* o_j = dev_out("C.cam_project.J", n_p * 6);
  double* o_uv = dev_out("C.cam_project.uv", n_p * 2);
  double* o_un = dev_out("C.cam_unproject", n_u * 3);
  double* o_pin = dev_out("C.unproject_pinhole", n_h * 3);
  int n = n_p;
  for (int v : {n_u, n_h}) n = v > n ? v : n;
  hipLaunchKernelGGL(k_cameras, dim3(blocks_of(n)), dim3(64), 0, 0, cams, n_p, pc, P, o_uvj, o_j, o_uv, n_u, uc, uvf, o_un,
                     n_h, hcam, uvd, o_pin);
  finish_family();
}

// ---------------------------------------------------------------- D. the visual edge
// per case: the frame's camera c0 and the rig (four cameras from rig[i] on) out of the camera table, the estimate
// (p, q), one observation (Xw, u, v, ur, inv_sigma2: float values; flags) and the Huber width.
// outputs: make_xf (Rcw, tcw, Rwb: 21); then (chi2, err[3], Pc[3]) of edge_error, J[18] of visual_jacobian,
// (chi2, err, Pc, J: 25) of edge_eval<false>, of edge_eval<true> forming its transform per edge, and of edge_eval<true>
// reading the table rig_cam_xf formed; (chi2, err, Pc) of edge_eval<true> without J; huber's (rho, rho') at that chi2
// and the 27 sums of visual_accumulate.
__device__ static void put25(double* o, double chi2, const double* err, const double* Pc, const double* J) {
  o[0] = chi2;
  for (int k = 0; k < 3; k++) o[1 + k] = err[k], o[4 + k] = Pc[k];
  for (int k = 0; k < 18; k++) o[7 + k] = J[k];
}
__global__ void k_visual(const CamD* cams, int n, const int* c0i, const int* rigi, const double* est, const double* obsf,
                         const int* flags, const double* delta, double* o_xf, double* o_ee, double* o_vj, double* o_ef,
                         double* o_et0, double* o_et1, double* o_etn, double* o_hub, double* o_acc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const CamD& c0 = cams[c0i[i]];
  const CamD* rig = cams + rigi[i];
  Est s;
  const double* e = est + i * 7;
  s.p[0] = e[0], s.p[1] = e[1], s.p[2] = e[2], s.qw = e[3], s.qx = e[4], s.qy = e[5], s.qz = e[6];
  vieo_pose_obs o;
  const double* f = obsf + i * 7;
  o.Xw[0] = (float)f[0], o.Xw[1] = (float)f[1], o.Xw[2] = (float)f[2];
  o.u = (float)f[3], o.v = (float)f[4], o.ur = (float)f[5], o.inv_sigma2 = (float)f[6], o.flags = flags[i];
  PoseXf X;
  make_xf(c0, s, X);
  for (int k = 0; k < 9; k++) o_xf[i * 21 + k] = X.Rcw[k], o_xf[i * 21 + 12 + k] = X.Rwb[k];
  for (int k = 0; k < 3; k++) o_xf[i * 21 + 9 + k] = X.tcw[k];
  double err[3], Pc[3], J[18];
  double chi2 = edge_error(c0, X, o, err, Pc);
  o_ee[i * 7] = chi2;
  for (int k = 0; k < 3; k++) o_ee[i * 7 + 1 + k] = err[k], o_ee[i * 7 + 4 + k] = Pc[k];
  visual_jacobian(c0, X, s.p, o, Pc, J);
  for (int k = 0; k < 18; k++) o_vj[i * 18 + k] = J[k];
  chi2 = edge_eval<false>(c0, rig, X, s.p, o, err, Pc, J);
  put25(o_ef + i * 25, chi2, err, Pc, J);
  const double d = delta[i];
  double r0, r1;
  huber(chi2, d, d * d, &r0, &r1);
  o_hub[i * 2] = r0, o_hub[i * 2 + 1] = r1;
  double acc[27];
  for (int k = 0; k < 27; k++) acc[k] = 0;
  visual_accumulate(J, err, (double)o.inv_sigma2, r1, o.ur >= 0, acc);
  for (int k = 0; k < 27; k++) o_acc[i * 27 + k] = acc[k];
  chi2 = edge_eval<true>(c0, rig, X, s.p, o, err, Pc, J);
  put25(o_et0 + i * 25, chi2, err, Pc, J);
  double xf[4 * 12];
  for (int c = 0; c < 4; c++) rig_cam_xf(rig[c], X, s.p, xf + c * 12);
  chi2 = edge_eval<true>(c0, rig, X, s.p, o, err, Pc, J, xf);
  put25(o_et1 + i * 25, chi2, err, Pc, J);
  chi2 = edge_eval<true>(c0, rig, X, s.p, o, err, Pc, nullptr);
  o_etn[i * 7] = chi2;
  for (int k = 0; k < 3; k++) o_etn[i * 7 + 1 + k] = err[k], o_etn[i * 7 + 4 + k] = Pc[k];
}

__global__ void k_huber(int n, const double* e, const double* delta, const double* dsqr, double* o) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double r0, r1;
  huber(e[i], delta[i], dsqr[i], &r0, &r1);
  o[i * 2] = r0, o[i * 2 + 1] = r1;
}

static void run_visual() {
  g_family = "D.visual_edge";
  int n_cams, n, m;
  const CamD* cams = upload_cameras(&n_cams);
  const int* c0 = dev_in<int>("D.cam0", 1, &n);
  const int* rig = dev_in<int>("D.rig", 1, &m);
  same_n("D.rig", n, m);
  {
    int64_t c;
    const int32_t* h0 = (const int32_t*)g_in.find("D.cam0", 1, &c);
    const int32_t* hr = (const int32_t*)g_in.find("D.rig", 1, &c);
    for (int i = 0; i < n; i++)
      if (h0[i] < 0 || h0[i] >= n_cams || hr[i] < 0 || hr[i] + 4 > n_cams) die("camera index out of range in", "D.cam0 / D.rig");
  }
  const double* est = dev_in<double>("D.pose", 7, &m);
  same_n("D.pose", n, m);
  const double* obs = dev_in<double>("D.obs", 7, &m);
  same_n("D.obs", n, m);
  const int* flags = dev_in<int>("D.flags", 1, &m);
  same_n("D.flags", n, m);
  const double* delta = dev_in<double>("D.delta", 1, &m);
  same_n("D.delta", n, m);
  double* o_xf = dev_out("D.make_xf", n * 21);
  double* o_ee = dev_out("D.edge_error", n * 7);
  double* o_vj = dev_out("D.visual_jacobian", n * 18);
  double* o_ef = dev_out("D.edge_eval<false>", n * 25);
  double* o_et0 = dev_out("D.edge_eval<true>", n * 25);
  double* o_et1 = dev_out("D.edge_eval<true>.table", n * 25);
  double* o_etn = dev_out("D.edge_eval<true>.no_J", n * 7);
  double* o_hub = dev_out("D.edge_huber", n * 2);
  double* o_acc = dev_out("D.visual_accumulate", n * 27);
  hipLaunchKernelGGL(k_visual, dim3(blocks_of(n)), dim3(64), 0, 0, cams, n, c0, rig, est, obs, flags, delta, o_xf, o_ee, o_vj,
                     o_ef, o_et0, o_et1, o_etn, o_hub, o_acc);
  finish_family();
  g_family = "D.huber";
  const double* he = dev_in<double>("D.huber_e", 1, &n);
  const double* hd = dev_in<double>("D.huber_delta", 1, &m);
  same_n("D.huber_delta", n, m);
  const double* hq = dev_in<double>("D.huber_dsqr", 1, &m);
  same_n("D.huber_dsqr", n, m);
  double* ho = dev_out("D.huber", n * 2);
  hipLaunchKernelGGL(k_huber, dim3(blocks_of(n)), dim3(64), 0, 0, n, he, hd, hq, ho);
  finish_family();
}

// ---------------------------------------------------------------- E. inertial and encoder edges
__device__ static void load_state(const double* e, NSd& s) {
  for (int k = 0; k < 3; k++)
    s.p[k] = e[k], s.v[k] = e[3 + k], s.bg[k] = e[10 + k], s.ba[k] = e[13 + k], s.dbg[k] = e[16 + k], s.dba[k] = e[19 + k];
  s.qw = e[6], s.qx = e[7], s.qy = e[8], s.qz = e[9];
}

// a measurement is the first 61 doubles of vieo_imu_preint: dt, Rij, vij, pij, JgR, Jgv, Jav, Jgp, Jap
__global__ void k_inertial(int n, const double* meas, const double* gw, const double* si, const double* sj, const int* idr,
                           double* o_err, double* o_err12, double* o_j, double* o_j12) {
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
  load_state(si + i * 22, a), load_state(sj + i * 22, b);
  const int idR = idr[i] == 3 ? 3 : 6, idV = 9 - idR;
  double err[9], err12[9];
  for (int k = 0; k < 9; k++) err[k] = 0, err12[k] = 0;
  imu_error(M, g, a, b, err, idR, 0);
  imu_error(M, g, a, b, err12, idR, 1);
  imu_error(M, g, a, b, err12, idR, 2);
  for (int k = 0; k < 9; k++) o_err[i * 9 + k] = err[k], o_err12[i * 9 + k] = err12[k];
  double J[9 * 24];
  imu_linearize(M, g, a, b, err, J, idR, idV, 0);
  for (int k = 0; k < 9 * 24; k++) o_j[i * 216 + k] = J[k];
  for (int k = 0; k < 9 * 24; k++) J[k] = 0;  // part 1 then part 2 into a cleared J
  imu_linearize(M, g, a, b, err, J, idR, idV, 1);
  imu_linearize(M, g, a, b, err, J, idR, idV, 2);
  for (int k = 0; k < 9 * 24; k++) o_j12[i * 216 + k] = J[k];
}

__global__ void k_encoder(int n, const double* si, const double* sj, const double* meas, const double* qbe,
                          const double* pbe, double* o_err, double* o_ji, double* o_jj, double* o_err_only) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  NSd a, b;
  load_state(si + i * 22, a), load_state(sj + i * 22, b);
  double m[6], q[4], p[3], err[6], Ji[36], Jj[36];
  for (int k = 0; k < 6; k++) m[k] = meas[i * 6 + k];
  for (int k = 0; k < 4; k++) q[k] = qbe[i * 4 + k];
  for (int k = 0; k < 3; k++) p[k] = pbe[i * 3 + k];
  enc_edge_eval(a, b, m, q, p, err, Ji, Jj);
  for (int k = 0; k < 6; k++) o_err[i * 6 + k] = err[k];
  for (int k = 0; k < 36; k++) o_ji[i * 36 + k] = Ji[k], o_jj[i * 36 + k] = Jj[k];
  enc_edge_eval(a, b, m, q, p, err, nullptr, nullptr);
  for (int k = 0; k < 6; k++) o_err_only[i * 6 + k] = err[k];
}

static void run_inertial() {
  g_family = "E.inertial";
  int n, m;
  const double* meas = dev_in<double>("E.imu_meas", 61, &n);
  const double* gw = dev_in<double>("E.imu_gw", 3, &m);
  same_n("E.imu_gw", n, m);
  const double* si = dev_in<double>("E.imu_si", 22, &m);
  same_n("E.imu_si", n, m);
  const double* sj = dev_in<double>("E.imu_sj", 22, &m);
  same_n("E.imu_sj", n, m);
  const int* idr = dev_in<int>("E.imu_idR", 1, &m);
  same_n("E.imu_idR", n, m);
  double* o_err = dev_out("E.imu_error", n * 9);
  double* o_err12 = dev_out("E.imu_error.parts", n * 9);
  double* o_j = dev_out("E.imu_linearize", (int64_t)n * 216);
  double* o_j12 = dev_out("E.imu_linearize.parts", (int64_t)n * 216);
  hipLaunchKernelGGL(k_inertial, dim3(blocks_of(n)), dim3(64), 0, 0, n, meas, gw, si, sj, idr, o_err, o_err12, o_j, o_j12);
  finish_family();
  g_family = "E.encoder";
  const double* esi = dev_in<double>("E.enc_si", 22, &n);
  const double* esj = dev_in<double>("E.enc_sj", 22, &m);
  same_n("E.enc_sj", n, m);
  const double* em = dev_in<double>("E.enc_meas", 6, &m);
  same_n("E.enc_meas", n, m);
  const double* eq = dev_in<double>("E.enc_qbe", 4, &m);
  same_n("E.enc_qbe", n, m);
  const double* ep = dev_in<double>("E.enc_pbe", 3, &m);
  same_n("E.enc_pbe", n, m);
  double* e_err = dev_out("E.enc_edge_eval.err", n * 6);
  double* e_ji = dev_out("E.enc_edge_eval.Ji", n * 36);
  double* e_jj = dev_out("E.enc_edge_eval.Jj", n * 36);
  double* e_only = dev_out("E.enc_edge_eval.err_only", n * 6);
  hipLaunchKernelGGL(k_encoder, dim3(blocks_of(n)), dim3(64), 0, 0, n, esi, esj, em, eq, ep, e_err, e_ji, e_jj, e_only);
  finish_family();
}

// ---------------------------------------------------------------- F. triangulation
// null_vector4<M> at the M the library instantiates: 4 (two observations), 8 (the fisheye stage's four cameras) and 16
// (eight observations of CreateNewMapPoints); A is [n][M][4], row-major
template <int M>
__global__ void k_null(int n, const double* A, double* o) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double a[M][4], x4[4];
  for (int r = 0; r < M; r++)
    for (int c = 0; c < 4; c++) a[r][c] = A[((size_t)i * M + r) * 4 + c];
  null_vector4<M>(a, x4);
  for (int c = 0; c < 4; c++) o[i * 4 + c] = x4[c];
}
template <int M>
static void null_one(const char* in_name, const char* out_name) {
  int n;
  const double* A = dev_in<double>(in_name, M * 4, &n);
  double* o = dev_out(out_name, n * 4);
  hipLaunchKernelGGL(k_null<M>, dim3(blocks_of(n)), dim3(64), 0, 0, n, A, o);
  finish_family();
}

// triangulate_matches_world<N>, N = 2 and 8 as tri_search.hip launches it; the slots live in global memory
template <int N>
__global__ void k_tri(int n, const TriObs* obs, const double* arg, const int* just, double* o) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const TriObs* mine = obs + (size_t)i * N;
  auto get = [mine](int k) { return mine[k]; };
  double X[3] = {arg[i * 4 + 1], arg[i * 4 + 2], arg[i * 4 + 3]};
  const bool ok = triangulate_matches_world<N>(get, (float)arg[i * 4], just[i] != 0, X);
  o[i * 4] = ok ? 1.0 : 0.0;
  for (int c = 0; c < 3; c++) o[i * 4 + 1 + c] = X[c];
}
// per slot: (on, camera) in i32 and (Tcw[12], nx, ny, u, v, sigma2, uright, bf) in f64; per case (thresh, x3d[3]) and
// just_check_p3d
template <int N>
static void tri_one(const CamD* cams, int n_cams, const char* si, const char* sf, const char* af, const char* ai,
                    const char* out_name) {
  int64_t ci, cf;
  const int32_t* hi = (const int32_t*)g_in.find(si, 1, &ci);
  const double* hf = (const double*)g_in.find(sf, 0, &cf);
  if (ci % (2 * N) || cf % (19 * N) || ci / (2 * N) != cf / (19 * N) || ci / (2 * N) > kMaxCases) die("slot tables", si);
  const int n = (int)(ci / (2 * N));
  double* tcw = nullptr;
  CK(hipMalloc(&tcw, (size_t)(n ? n : 1) * N * 12 * 8));
  std::vector<double> ht((size_t)n * N * 12);
  std::vector<TriObs> ho((size_t)n * N);
  for (int k = 0; k < n * N; k++) {
    const double* f = hf + (size_t)k * 19;
    for (int c = 0; c < 12; c++) ht[(size_t)k * 12 + c] = f[c];
    if (hi[k * 2 + 1] < 0 || hi[k * 2 + 1] >= n_cams) die("camera index out of range in", si);
    TriObs& t = ho[k];
    t.on = hi[k * 2] != 0, t.cam = cams + hi[k * 2 + 1], t.Tcw = tcw + (size_t)k * 12;
    t.nx = f[12], t.ny = f[13], t.u = (float)f[14], t.v = (float)f[15], t.sigma2 = (float)f[16];
    t.uright = (float)f[17], t.bf = (float)f[18];
  }
  if (n) CK(hipMemcpy(tcw, ht.data(), ht.size() * 8, hipMemcpyHostToDevice));
  TriObs* obs = nullptr;
  CK(hipMalloc(&obs, (ho.size() ? ho.size() : 1) * sizeof(TriObs)));
  if (n) CK(hipMemcpy(obs, ho.data(), ho.size() * sizeof(TriObs), hipMemcpyHostToDevice));
  int m;
  const double* arg = dev_in<double>(af, 4, &m);
  same_n(af, n, m);
  const int* just = dev_in<int>(ai, 1, &m);
  same_n(ai, n, m);
  double* o = dev_out(out_name, n * 4);
  hipLaunchKernelGGL(k_tri<N>, dim3(blocks_of(n)), dim3(64), 0, 0, n, obs, arg, just, o);
  finish_family();
}

static void run_triangulation() {
  g_family = "F.null_vector4";
  null_one<4>("F.null4_A", "F.null_vector4<4>");
  null_one<8>("F.null8_A", "F.null_vector4<8>");
  null_one<16>("F.null16_A", "F.null_vector4<16>");
  g_family = "F.triangulate";
  int n_cams;
  const CamD* cams = upload_cameras(&n_cams);
  tri_one<2>(cams, n_cams, "F.tri2_slot_i32", "F.tri2_slot_f64", "F.tri2_arg_f64", "F.tri2_arg_i32", "F.triangulate<2>");
  tri_one<8>(cams, n_cams, "F.tri8_slot_i32", "F.tri8_slot_f64", "F.tri8_arg_f64", "F.tri8_arg_i32", "F.triangulate<8>");
}

// ---------------------------------------------------------------- G. reductions
// pool: [2 data sets][n_blocks][256 threads][28 values]; a <N, BS> instance sums values 0..N-1 of threads 0..BS-1.
// Each function is called twice in a row, on data set 0 and then on data set 1, and every thread writes what it holds
// after each call: out[data set][block][thread][N].
constexpr int kPoolT = 256, kPoolN = 28;
template <int KIND, int N, int BS>
__global__ void __launch_bounds__(BS) k_reduce(const double* pool, double* out) {
  __shared__ double s_red[KIND == 2 ? N * (BS / 32) * 34 : 4 * N];
  __shared__ double s_out[N];
  const int tid = threadIdx.x, b = blockIdx.x, nb = gridDim.x;
  for (int ds = 0; ds < 2; ds++) {
    double v[N];
    const double* src = pool + ((size_t)(ds * nb + b) * kPoolT + tid) * kPoolN;
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = src[i];
    double* dst = out + ((size_t)(ds * nb + b) * BS + tid) * N;
    if (KIND == 0) {
      block_sum<N>(v, s_red, tid);
#pragma unroll
      for (int i = 0; i < N; i++) dst[i] = v[i];
    } else if (KIND == 1) {
      block_sum_bs<N, BS>(v, s_red, tid);
#pragma unroll
      for (int i = 0; i < N; i++) dst[i] = v[i];
    } else {
      block_sum_lds<N, BS>(v, s_red, s_out, tid);
      for (int i = 0; i < N; i++) dst[i] = s_out[i];
    }
  }
}

template <int KIND, int N, int BS>
static void reduce_one(const char* name, const double* pool, int nb) {
  static_assert(N <= kPoolN && BS <= kPoolT, "inside the pool");
  double* o = dev_out(name, (int64_t)2 * nb * BS * N);
  hipLaunchKernelGGL((k_reduce<KIND, N, BS>), dim3(nb), dim3(BS), 0, 0, pool, o);
  finish_family();
}

static void run_reductions() {
  g_family = "G.reductions";
  int64_t count;
  const double* h = (const double*)g_in.find("G.pool", 0, &count);
  const int64_t per = (int64_t)2 * kPoolT * kPoolN;
  if (count % per || count / per < 1 || count / per > 64) die("1 .. 64 blocks in", "G.pool");
  const int nb = (int)(count / per);
  double* pool = nullptr;
  CK(hipMalloc(&pool, (size_t)count * 8));
  CK(hipMemcpy(pool, h, (size_t)count * 8, hipMemcpyHostToDevice));
  reduce_one<0, 1, 256>("G.block_sum<1>", pool, nb);
  reduce_one<0, 2, 256>("G.block_sum<2>", pool, nb);
  reduce_one<0, 3, 256>("G.block_sum<3>", pool, nb);
  reduce_one<0, 6, 256>("G.block_sum<6>", pool, nb);
  reduce_one<0, 27, 256>("G.block_sum<27>", pool, nb);
  reduce_one<1, 1, 64>("G.block_sum_bs<1,64>", pool, nb);
  reduce_one<1, 27, 64>("G.block_sum_bs<27,64>", pool, nb);
  reduce_one<1, 1, 256>("G.block_sum_bs<1,256>", pool, nb);
  reduce_one<1, 27, 256>("G.block_sum_bs<27,256>", pool, nb);
  reduce_one<2, 28, 64>("G.block_sum_lds<28,64>", pool, nb);
  reduce_one<2, 28, 256>("G.block_sum_lds<28,256>", pool, nb);
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
    return 2;
  }
  g_in.load(argv[1]);
  run_rotations();
  run_retractions();
  run_cameras();
  run_visual();
  run_inertial();
  run_triangulation();
  run_reductions();
  g_family = "output";
  g_out.write(argv[2]);
  return 0;
}
