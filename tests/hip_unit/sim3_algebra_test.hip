// Stand-alone evaluator of the Sim3 algebra of the pose graph (built and run by tests/test_sim3_algebra.py):
// sim3_device.h, and the state functions, Huber and the small LDL^T of sim3_optimize_device.h, as hipcc compiles them
// for the device -- the device's libm, the library's flags.  One __global__ kernel per
// family with one lane per case.  Nothing is compared here: the program reads named arrays, evaluates, writes named
// arrays.
//
//   sim3_algebra_test in.bin out.bin
//
// The files have the layout of device_algebra_test.hip: char magic[8] = "VIEOALG1"; int32 n_entries; int32 reserved;
// n_entries x { char name[32]; int32 dtype (0 = f64, 1 = i32); int32 reserved; int64 count; int64 byte_offset; }; the
// arrays.  Every output is f64.
//
// The taps (S3_TAP of sim3_device.h, kTapSlots doubles per case): 0 / 1 the branch and the trace of s3_mat_to_quat,
// 2 / 3 / 4 theta < eps, theta and |sigma| < eps of s3_exp, 5 / 6 / 7 / 8 d > 1 - eps, d, |sigma| < eps and sigma of
// s3_log, 9 / 10 theta < 1e-5 and theta of s3o_inc_small.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static const int kTapSlots = 12;
__device__ double* g_s3_tap;  // [case][kTapSlots]; null while a family without taps runs
__host__ __device__ inline void s3_tap_write(int slot, double value) {
#ifdef __HIP_DEVICE_COMPILE__
  if (g_s3_tap) g_s3_tap[(size_t)(blockIdx.x * blockDim.x + threadIdx.x) * kTapSlots + slot] = value;
#else
  (void)slot, (void)value;
#endif
}
#define S3_TAP(slot, value) s3_tap_write(slot, value);

#include "../../vieo_slam_amd/csrc/sim3_device.h"
#include "../../vieo_slam_amd/csrc/sim3_optimize_device.h"

using namespace vieo;
static_assert(sizeof(Sim3) == 64, "Sim3 is eight doubles");
static_assert(sizeof(S3oState) == 64, "S3oState is eight doubles");

// ---------------------------------------------------------------- files
struct Entry {
  char name[32];
  int32_t dtype, reserved;
  int64_t count, offset;
};
static_assert(sizeof(Entry) == 56, "table of contents entry");

static const char* g_family = "input";
[[noreturn]] static void die(const char* what, const char* detail) {
  fprintf(stderr, "sim3_algebra_test: family %s: %s: %s\n", g_family, what, detail);
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
  const double* find(const char* name, int64_t* count) const {
    for (const Entry& e : toc)
      if (!strncmp(e.name, name, 32)) {
        if (e.dtype != 0) die("dtype of", name);
        *count = e.count;
        return (const double*)(bytes.data() + e.offset);
      }
    die("missing array", name);
  }
};

struct Out {
  std::vector<Entry> toc;
  std::vector<std::vector<char>> data;
  void add(const char* name, const double* p, int64_t count) {
    Entry e;
    memset(&e, 0, sizeof(e));
    strncpy(e.name, name, 31);
    e.dtype = 0, e.count = count;
    toc.push_back(e);
    data.emplace_back((const char*)p, (const char*)p + (size_t)count * 8);
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

// input array `name` (n rows of `per` doubles) on the device; n comes back
static const double* dev_in(const char* name, int per, int* n) {
  int64_t count;
  const double* h = g_in.find(name, &count);
  if (count % per) die("row length of", name);
  if (count / per > kMaxCases) die("more than 4096 cases in", name);
  *n = (int)(count / per);
  double* d = nullptr;
  CK(hipMalloc(&d, (size_t)(count ? count : 1) * 8));
  if (count) CK(hipMemcpy(d, h, (size_t)count * 8, hipMemcpyHostToDevice));
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
static inline int blocks_of(int n) { return n > 0 ? (n + 63) / 64 : 1; }
// the tap area of a family of n cases: every lane of the launch has its row, so a lane past n could write too
static void set_tap(const char* name, int n) {
  double* t = name ? dev_out(name, (int64_t)blocks_of(n) * 64 * kTapSlots) : nullptr;
  CK(hipMemcpyToSymbol(HIP_SYMBOL(g_s3_tap), &t, sizeof(t)));
}
static void finish_family() {
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  for (const DevOut& o : g_pending) {
    std::vector<double> h((size_t)o.count);
    if (o.count) CK(hipMemcpy(h.data(), o.d, (size_t)o.count * 8, hipMemcpyDeviceToHost));
    g_out.add(o.name, h.data(), o.count);
  }
  g_pending.clear();
}

// ---------------------------------------------------------------- the families
__device__ inline Sim3 load_sim3(const double* p) {
  Sim3 S;
  for (int k = 0; k < 4; k++) S.q[k] = p[k];
  for (int k = 0; k < 3; k++) S.t[k] = p[4 + k];
  S.s = p[7];
  return S;
}
__device__ inline void store_sim3(const Sim3& S, double* p) {
  for (int k = 0; k < 4; k++) p[k] = S.q[k];
  for (int k = 0; k < 3; k++) p[4 + k] = S.t[k];
  p[7] = S.s;
}

__global__ void k_quat_to_mat(int n, const double* q, double* R) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double o[9];
  s3_quat_to_mat(q + 4 * (size_t)i, o);
  for (int k = 0; k < 9; k++) R[9 * (size_t)i + k] = o[k];
}
__global__ void k_mat_to_quat(int n, const double* R, double* q) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double m[9], o[4];
  for (int k = 0; k < 9; k++) m[k] = R[9 * (size_t)i + k];
  s3_mat_to_quat(m, o);
  for (int k = 0; k < 4; k++) q[4 * (size_t)i + k] = o[k];
}
__global__ void k_quat_rot(int n, const double* q, const double* v, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double o[3];
  s3_quat_rot(q + 4 * (size_t)i, v + 3 * (size_t)i, o);
  for (int k = 0; k < 3; k++) out[3 * (size_t)i + k] = o[k];
}
__global__ void k_mul(int n, const double* a, const double* b, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  store_sim3(s3_mul(load_sim3(a + 8 * (size_t)i), load_sim3(b + 8 * (size_t)i)), out + 8 * (size_t)i);
}
__global__ void k_inverse(int n, const double* a, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  store_sim3(s3_inverse(load_sim3(a + 8 * (size_t)i)), out + 8 * (size_t)i);
}
__global__ void k_map(int n, const double* a, const double* p, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double o[3];
  s3_map(load_sim3(a + 8 * (size_t)i), p + 3 * (size_t)i, o);
  for (int k = 0; k < 3; k++) out[3 * (size_t)i + k] = o[k];
}
__global__ void k_exp(int n, const double* u, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double w[7];
  for (int k = 0; k < 7; k++) w[k] = u[7 * (size_t)i + k];
  store_sim3(s3_exp(w), out + 8 * (size_t)i);
}
__global__ void k_log(int n, const double* S, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double r[7];
  s3_log(load_sim3(S + 8 * (size_t)i), r);
  for (int k = 0; k < 7; k++) out[7 * (size_t)i + k] = r[k];
}
__global__ void k_edge_error(int n, const double* C, const double* Si, const double* Sj, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double r[7];
  s3_edge_error(load_sim3(C + 8 * (size_t)i), load_sim3(Si + 8 * (size_t)i), load_sim3(Sj + 8 * (size_t)i), r);
  for (int k = 0; k < 7; k++) out[7 * (size_t)i + k] = r[k];
}

// ---- sim3_optimize_device.h: a state travels as p[3], q[4], s
__device__ inline S3oState load_state(const double* p) {
  S3oState S;
  for (int k = 0; k < 3; k++) S.p[k] = p[k];
  for (int k = 0; k < 4; k++) S.q[k] = p[3 + k];
  S.s = p[7];
  return S;
}
__device__ inline void store_state(const S3oState& S, double* p) {
  for (int k = 0; k < 3; k++) p[k] = S.p[k];
  for (int k = 0; k < 4; k++) p[3 + k] = S.q[k];
  p[7] = S.s;
}
__global__ void k_quat_normalize(int n, const double* q, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double o[4];
  for (int k = 0; k < 4; k++) o[k] = q[4 * (size_t)i + k];
  s3o_quat_normalize(o);
  for (int k = 0; k < 4; k++) out[4 * (size_t)i + k] = o[k];
}
__global__ void k_state_from_sim3(int n, const double* Rts, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double R[9], t[3];
  for (int k = 0; k < 9; k++) R[k] = Rts[13 * (size_t)i + k];
  for (int k = 0; k < 3; k++) t[k] = Rts[13 * (size_t)i + 9 + k];
  S3oState S;
  s3o_state_from_sim3(R, t, Rts[13 * (size_t)i + 12], S);
  store_state(S, out + 8 * (size_t)i);
}
__global__ void k_state_to_sim3(int n, const double* st, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double R[9], t[3], s;
  s3o_state_to_sim3(load_state(st + 8 * (size_t)i), R, t, &s);
  for (int k = 0; k < 9; k++) out[13 * (size_t)i + k] = R[k];
  for (int k = 0; k < 3; k++) out[13 * (size_t)i + 9 + k] = t[k];
  out[13 * (size_t)i + 12] = s;
}
__global__ void k_inc_small(int n, const double* st, const double* d, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  S3oState S = load_state(st + 8 * (size_t)i);
  double inc[7];
  for (int k = 0; k < 7; k++) inc[k] = d[8 * (size_t)i + k];
  s3o_inc_small(S, inc, d[8 * (size_t)i + 7] != 0.0);
  store_state(S, out + 8 * (size_t)i);
}
__device__ inline CamD cam_of(const double* c) {  // model, num_k, fx, fy, cx, cy, k[8], Rcb[9], tcb[3]
  CamD d;
  d.model = (int)c[0], d.num_k = (int)c[1];
  d.fx = c[2], d.fy = c[3], d.cx = c[4], d.cy = c[5], d.bf = 0;
  for (int i = 0; i < 8; i++) d.k[i] = c[6 + i];
  for (int i = 0; i < 9; i++) d.Rcb[i] = c[14 + i];
  for (int i = 0; i < 3; i++) d.tcb[i] = c[23 + i];
  return d;
}
// in = mode, camera, q[4], p[3], s, X[3], obs[2]; out = e[2] and J[14] of the call with J, e[2] of the call without
__global__ void k_edge(int n, const double* in, const double* cams, int n_cams, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double a[15];
  for (int k = 0; k < 15; k++) a[k] = in[15 * (size_t)i + k];
  const int ci = (int)a[1];
  if (ci < 0 || ci >= n_cams) return;
  const CamD c = cam_of(cams + 26 * (size_t)ci);
  double Rwb[9], e[2], J[14], e2[2];
  s3_quat_to_mat(a + 2, Rwb);
  if (a[0] == 1.0) {
    s3o_edge<1>(c, Rwb, a + 6, a[9], a + 10, a + 13, e, J);
    s3o_edge<1>(c, Rwb, a + 6, a[9], a + 10, a + 13, e2, nullptr);
  } else {
    s3o_edge<2>(c, Rwb, a + 6, a[9], a + 10, a + 13, e, J);
    s3o_edge<2>(c, Rwb, a + 6, a[9], a + 10, a + 13, e2, nullptr);
  }
  double* o = out + 18 * (size_t)i;
  o[0] = e[0], o[1] = e[1], o[16] = e2[0], o[17] = e2[1];
  for (int k = 0; k < 14; k++) o[2 + k] = J[k];
}
// in = e[2], J[14], info, delta, dsqr; out = the 36 accumulators from zero, s3o_chi2
__global__ void k_add_edge(int n, const double* in, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double a[19], acc[36];
  for (int k = 0; k < 19; k++) a[k] = in[19 * (size_t)i + k];
  for (int k = 0; k < 36; k++) acc[k] = 0;
  const double chi2 = s3o_chi2(a, a[16]);
  s3o_add_edge(a, a + 2, a[16], chi2, a[17], a[18], acc);
  for (int k = 0; k < 36; k++) out[37 * (size_t)i + k] = acc[k];
  out[37 * (size_t)i + 36] = chi2;
}
__global__ void k_huber(int n, const double* in, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double r0, r1;
  s3o_huber(in[3 * (size_t)i], in[3 * (size_t)i + 1], in[3 * (size_t)i + 2], &r0, &r1);
  out[2 * (size_t)i] = r0, out[2 * (size_t)i + 1] = r1;
}
__global__ void k_ldlt(int n, const double* in, double* out) {  // in = acc[36], lambda, N; out = ok, x[7] (x starts as a guard)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double acc[36], x[7];
  for (int k = 0; k < 36; k++) acc[k] = in[38 * (size_t)i + k];
  for (int k = 0; k < 7; k++) x[k] = -7.0;
  const double lambda = in[38 * (size_t)i + 36];
  const bool ok = in[38 * (size_t)i + 37] == 6.0 ? s3o_ldlt_solve<6>(acc, lambda, x) : s3o_ldlt_solve<7>(acc, lambda, x);
  out[8 * (size_t)i] = ok ? 1.0 : 0.0;
  for (int k = 0; k < 7; k++) out[8 * (size_t)i + 1 + k] = x[k];
}

static void run_unary(const char* family, void (*kern)(int, const double*, double*), const char* in, int per_in, const char* out,
                      int per_out, const char* tap) {
  g_family = family;
  int n;
  const double* a = dev_in(in, per_in, &n);
  double* o = dev_out(out, (int64_t)n * per_out);
  set_tap(tap, n);
  hipLaunchKernelGGL(kern, dim3(blocks_of(n)), dim3(64), 0, 0, n, a, o);
  finish_family();
}
static void run_binary(const char* family, void (*kern)(int, const double*, const double*, double*), const char* in_a, int per_a,
                       const char* in_b, int per_b, const char* out, int per_out) {
  g_family = family;
  int n, n2;
  const double* a = dev_in(in_a, per_a, &n);
  const double* b = dev_in(in_b, per_b, &n2);
  same_n(in_b, n, n2);
  double* o = dev_out(out, (int64_t)n * per_out);
  set_tap(nullptr, n);
  hipLaunchKernelGGL(kern, dim3(blocks_of(n)), dim3(64), 0, 0, n, a, b, o);
  finish_family();
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: sim3_algebra_test in.bin out.bin\n");
    return 2;
  }
  g_in.load(argv[1]);
  run_unary("quat_to_mat", k_quat_to_mat, "G.quat", 4, "G.s3_quat_to_mat", 9, nullptr);
  run_unary("mat_to_quat", k_mat_to_quat, "G.mat", 9, "G.s3_mat_to_quat", 4, "G.mat_to_quat.tap");
  run_binary("quat_rot", k_quat_rot, "G.rot_q", 4, "G.rot_v", 3, "G.s3_quat_rot", 3);
  run_binary("mul", k_mul, "G.mul_a", 8, "G.mul_b", 8, "G.s3_mul", 8);
  run_unary("inverse", k_inverse, "G.sim3", 8, "G.s3_inverse", 8, nullptr);
  run_binary("map", k_map, "G.map_S", 8, "G.map_p", 3, "G.s3_map", 3);
  run_unary("exp", k_exp, "X.u", 7, "X.s3_exp", 8, "X.tap");
  run_unary("log", k_log, "L.S", 8, "L.s3_log", 7, "L.tap");
  run_unary("log near pi", k_log, "P.S", 8, "P.s3_log", 7, "P.tap");
  {
    g_family = "edge_error";
    int n, n2, n3;
    const double* C = dev_in("E.C", 8, &n);
    const double* Si = dev_in("E.Si", 8, &n2);
    const double* Sj = dev_in("E.Sj", 8, &n3);
    same_n("E.Si", n, n2), same_n("E.Sj", n, n3);
    double* o = dev_out("E.s3_edge_error", (int64_t)n * 7);
    set_tap("E.tap", n);
    hipLaunchKernelGGL(k_edge_error, dim3(blocks_of(n)), dim3(64), 0, 0, n, C, Si, Sj, o);
    finish_family();
  }
  run_unary("quat_normalize", k_quat_normalize, "O.raw_quat", 4, "O.s3o_quat_normalize", 4, nullptr);
  run_unary("state_from_sim3", k_state_from_sim3, "O.Rts", 13, "O.s3o_state_from_sim3", 8, nullptr);
  run_unary("state_to_sim3", k_state_to_sim3, "O.state", 8, "O.s3o_state_to_sim3", 13, nullptr);
  {
    g_family = "inc_small";
    int n, n2;
    const double* st = dev_in("O.inc_state", 8, &n);
    const double* d = dev_in("O.inc_d", 8, &n2);
    same_n("O.inc_d", n, n2);
    double* o = dev_out("O.s3o_inc_small", (int64_t)n * 8);
    set_tap("O.inc_small.tap", n);
    hipLaunchKernelGGL(k_inc_small, dim3(blocks_of(n)), dim3(64), 0, 0, n, st, d, o);
    finish_family();
  }
  {
    g_family = "edge";
    int n, nc;
    const double* in = dev_in("O.edge", 15, &n);
    const double* cams = dev_in("O.cams", 26, &nc);
    double* o = dev_out("O.s3o_edge", (int64_t)n * 18);
    set_tap(nullptr, n);
    hipLaunchKernelGGL(k_edge, dim3(blocks_of(n)), dim3(64), 0, 0, n, in, cams, nc, o);
    finish_family();
  }
  run_unary("add_edge", k_add_edge, "O.add_edge", 19, "O.s3o_add_edge", 37, nullptr);
  run_unary("huber", k_huber, "O.huber", 3, "O.s3o_huber", 2, nullptr);
  run_unary("ldlt", k_ldlt, "O.ldlt", 38, "O.s3o_ldlt_solve", 8, nullptr);
  g_out.write(argv[2]);
  return 0;
}
