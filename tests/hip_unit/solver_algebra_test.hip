// Stand-alone evaluator of the lane functions of the relocalisation and loop-verification solvers (built and run by
// tests/test_solver_algebra.py): pnp_device.h (EPnP and CheckInliers of PnPsolver) and sim3_solver_device.h (Horn's
// method and CheckInliers of Sim3Solver), with cam_project.h for the CamD of s3s_project.  One __global__ kernel per
// family with one lane per case; pnp_epnp runs in its real shape: workgroups of kPnpLanes = 16 lanes, each with the two
// __shared__ double[144 * 16] work arrays, one job per lane, the last workgroup partly filled.  Built with the
// library's flags.  Nothing is compared here: the program reads named arrays, evaluates, writes named arrays.
//
//   solver_algebra_test in.bin out.bin
//
// The files have the layout of device_algebra_test.hip: char magic[8] = "VIEOALG1"; int32 n_entries; int32 reserved;
// n_entries x { char name[32]; int32 dtype (0 = f64, 1 = i32); int32 reserved; int64 count; int64 byte_offset; }; the
// arrays.  Float inputs travel as the doubles they widen to.  Every output is f64.
//
// pnp_epnp's taps (PNP_TAP of pnp_device.h, 48 doubles per job): 0-3 the four chosen eigenvalues, 4-9 rho,
// 10 + 4 (variant - 1) ... the initial betas of the variant, 21 + variant its reprojection error, 24 + variant z0 of
// solve_for_sign, 27 + variant det R before the flip, 31-34 / 35-37 / 38-42 the least-squares x of variants 1 / 2 / 3.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static const int kTapSlots = 48;
__device__ double* g_pnp_tap;  // [job][kTapSlots]
#define PNP_TAP(slot, value) g_pnp_tap[(size_t)(blockIdx.x * 16 + lane) * kTapSlots + (slot)] = (value);

#include "../../vieo_slam_amd/csrc/cam_project.h"
#include "../../vieo_slam_amd/csrc/pnp_device.h"
#include "../../vieo_slam_amd/csrc/sim3_solver_device.h"

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
  fprintf(stderr, "solver_algebra_test: family %s: %s: %s\n", g_family, what, detail);
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

// the host copy of input array `name` (count = n * per); n comes back
template <class T>
static const T* host_in(const char* name, int per, int* n) {
  int64_t count;
  const void* h = g_in.find(name, sizeof(T) == 8 ? 0 : 1, &count);
  if (count % per) die("row length of", name);
  if (count / per > kMaxCases * 64) die("too many rows in", name);
  *n = (int)(count / per);
  return (const T*)h;
}
template <class T>
static const T* to_dev(const T* h, size_t count) {
  T* d = nullptr;
  CK(hipMalloc(&d, (count ? count : 1) * sizeof(T)));
  if (count) CK(hipMemcpy(d, h, count * sizeof(T), hipMemcpyHostToDevice));
  return d;
}
// input array `name` on the device
template <class T>
static const T* dev_in(const char* name, int per, int* n) {
  const T* h = host_in<T>(name, per, n);
  if (*n > kMaxCases) die("more than 4096 cases in", name);
  return to_dev(h, (size_t)*n * per);
}
// float data sent as doubles: narrowed on the host (exact: they are floats)
static const float* dev_in_float(const char* name, int per, int* n) {
  const double* h = host_in<double>(name, per, n);
  std::vector<float> f((size_t)*n * per);
  for (size_t i = 0; i < f.size(); i++) f[i] = (float)h[i];
  return to_dev(f.data(), f.size());
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
    g_out.add(o.name, h.data(), o.count);
  }
  g_pending.clear();
}
static inline int blocks_of(int n) { return n > 0 ? (n + 63) / 64 : 1; }

// ---------------------------------------------------------------- L. pnp_lstsq6<3 | 4 | 5>
template <int NC>
__global__ void k_lstsq(int n, const double* Ain, const double* bin, double* x_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double A[6][NC], b[6], x[NC];
  for (int r = 0; r < 6; r++) {
    for (int c = 0; c < NC; c++) A[r][c] = Ain[(size_t)i * 6 * NC + r * NC + c];
    b[r] = bin[(size_t)i * 6 + r];
  }
  pnp_lstsq6<NC>(A, b, x);
  for (int c = 0; c < NC; c++) x_out[(size_t)i * NC + c] = x[c];
}

template <int NC>
static void run_lstsq(const char* nA, const char* nb, const char* nx) {
  int n, n2;
  const double* A = dev_in<double>(nA, 6 * NC, &n);
  const double* b = dev_in<double>(nb, 6, &n2);
  same_n(nb, n, n2);
  double* x = dev_out(nx, (int64_t)n * NC);
  hipLaunchKernelGGL(k_lstsq<NC>, dim3(blocks_of(n)), dim3(64), 0, 0, n, A, b, x);
  finish_family();
}

// ---------------------------------------------------------------- R. pnp_rot, E. pnp_eig3, P. pnp_polar3
__global__ void k_small(int n_r, const double* abg, double* o_rot, int n_e, const double* S, double* o_d, double* o_U,
                        int n_p, const double* B, double* o_R) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_r) {
    double t, cs, sn;
    pnp_rot(abg[i * 3], abg[i * 3 + 1], abg[i * 3 + 2], t, cs, sn);
    o_rot[i * 3] = t, o_rot[i * 3 + 1] = cs, o_rot[i * 3 + 2] = sn;
  }
  if (i < n_e) {
    double M[3][3], d[3], U[3][3];
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) M[r][c] = S[i * 9 + r * 3 + c];
    pnp_eig3(M, d, U);
    for (int r = 0; r < 3; r++) {
      o_d[i * 3 + r] = d[r];
      for (int c = 0; c < 3; c++) o_U[i * 9 + r * 3 + c] = U[r][c];
    }
  }
  if (i < n_p) {
    double M[3][3], R[3][3];
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) M[r][c] = B[i * 9 + r * 3 + c];
    pnp_polar3(M, R);
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) o_R[i * 9 + r * 3 + c] = R[r][c];
  }
}

static void run_small() {
  g_family = "R/E/P.small";
  int n_r, n_e, n_p;
  const double* abg = dev_in<double>("R.abg", 3, &n_r);
  const double* S = dev_in<double>("E.S", 9, &n_e);
  const double* B = dev_in<double>("P.B", 9, &n_p);
  double* o_rot = dev_out("R.pnp_rot", n_r * 3);
  double* o_d = dev_out("E.pnp_eig3.d", n_e * 3);
  double* o_U = dev_out("E.pnp_eig3.U", n_e * 9);
  double* o_R = dev_out("P.pnp_polar3", n_p * 9);
  int n = n_r > n_e ? n_r : n_e;
  n = n_p > n ? n_p : n;
  hipLaunchKernelGGL(k_small, dim3(blocks_of(n)), dim3(64), 0, 0, n_r, abg, o_rot, n_e, S, o_d, o_U, n_p, B, o_R);
  finish_family();
}

// ---------------------------------------------------------------- Q. pnp_alphas, pnp_project
static __device__ PnpCandDev cand_of(const double* K, int off, int n) {
  PnpCandDev C;
  C.off = off, C.n = n, C.fx = (float)K[0], C.fy = (float)K[1], C.cx = (float)K[2], C.cy = (float)K[3];
  C.words = (n + 63) / 64, C.mask_off = 0;
  return C;
}

__global__ void k_points(int n_a, const double* frame, const float* Xa, double* o_a, int n_j, const double* K,
                         const double* Rt, const float* Xj, double* o_uv) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_a) {
    PnpFrame F;
    for (int r = 0; r < 3; r++) {
      F.c0[r] = frame[i * 12 + r];
      for (int c = 0; c < 3; c++) F.ci[r][c] = frame[i * 12 + 3 + r * 3 + c];
    }
    double a[4];
    pnp_alphas(F, Xa + i * 3, a);
    for (int k = 0; k < 4; k++) o_a[i * 4 + k] = a[k];
  }
  if (i < n_j) {
    const PnpCandDev C = cand_of(K + i * 4, 0, 1);
    double R[3][3], t[3], ue, ve;
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) R[r][c] = Rt[i * 12 + r * 3 + c];
      t[r] = Rt[i * 12 + 9 + r];
    }
    pnp_project(C, R, t, Xj + i * 3, ue, ve);
    o_uv[i * 2] = ue, o_uv[i * 2 + 1] = ve;
  }
}

static void run_points() {
  g_family = "Q.points";
  int n_a, n_a2, n_j, n_j2, n_j3;
  const double* frame = dev_in<double>("Q.frame", 12, &n_a);
  const float* Xa = dev_in_float("Q.X", 3, &n_a2);
  same_n("Q.X", n_a, n_a2);
  const double* K = dev_in<double>("J.K", 4, &n_j);
  const double* Rt = dev_in<double>("J.Rt", 12, &n_j2);
  const float* Xj = dev_in_float("J.X", 3, &n_j3);
  same_n("J.Rt", n_j, n_j2), same_n("J.X", n_j, n_j3);
  double* o_a = dev_out("Q.pnp_alphas", n_a * 4);
  double* o_uv = dev_out("J.pnp_project", n_j * 2);
  const int n = n_a > n_j ? n_a : n_j;
  hipLaunchKernelGGL(k_points, dim3(blocks_of(n)), dim3(64), 0, 0, n_a, frame, Xa, o_a, n_j, K, Rt, Xj, o_uv);
  finish_family();
}

// ---------------------------------------------------------------- I. pnp_check_inliers
// a case is (off, n, fill) in i32 -- fill != 0: its mask words hold ones before the call --, K[4] and Rt[12] in f64; the
// points of all cases are concatenated.  A mask has kMaskWords words; those beyond the case's own are never written and
// come back as the guard value they were given.
static const int kMaskWords = 4;
__global__ void k_check(int n, const int* cs, const double* K, const double* Rt, const float* Xw, const float* uv,
                        const float* me, unsigned long long* mask, double* o_count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const PnpCandDev C = cand_of(K + i * 4, cs[i * 3], cs[i * 3 + 1]);
  double R[3][3], t[3];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) R[r][c] = Rt[i * 12 + r * 3 + c];
    t[r] = Rt[i * 12 + 9 + r];
  }
  o_count[i] = pnp_check_inliers(C, Xw, uv, me, R, t, mask + (size_t)i * kMaskWords);
}

static void run_check() {
  g_family = "I.check_inliers";
  int n, n2, n3, np, np2, np3;
  const int* cs_h = host_in<int32_t>("I.case", 3, &n);
  const double* K = dev_in<double>("I.K", 4, &n2);
  const double* Rt = dev_in<double>("I.Rt", 12, &n3);
  same_n("I.K", n, n2), same_n("I.Rt", n, n3);
  if (n > kMaxCases) die("more than 4096 cases in", "I.case");
  const float* Xw = dev_in_float("I.Xw", 3, &np);
  const float* uv = dev_in_float("I.uv", 2, &np2);
  const float* me = dev_in_float("I.max_err", 1, &np3);
  same_n("I.uv", np, np2), same_n("I.max_err", np, np3);
  std::vector<unsigned long long> words((size_t)(n ? n : 1) * kMaskWords);
  for (int i = 0; i < n; i++) {
    const int off = cs_h[i * 3], cnt = cs_h[i * 3 + 1];
    if (off < 0 || cnt < 0 || off + cnt > np || (cnt + 63) / 64 >= kMaskWords) die("case outside the points", "I.case");
    for (int w = 0; w < kMaskWords; w++)
      words[(size_t)i * kMaskWords + w] = w >= (cnt + 63) / 64 ? 0x5A5A5A5A5A5A5A5Aull : cs_h[i * 3 + 2] ? ~0ull : 0ull;
  }
  const int* cs = to_dev(cs_h, (size_t)n * 3);
  unsigned long long* mask = (unsigned long long*)to_dev(words.data(), words.size());
  double* o_count = dev_out("I.count", n);
  hipLaunchKernelGGL(k_check, dim3(blocks_of(n)), dim3(64), 0, 0, n, cs, K, Rt, Xw, uv, me, mask, o_count);
  finish_family();
  CK(hipMemcpy(words.data(), mask, words.size() * 8, hipMemcpyDeviceToHost));
  std::vector<double> halves((size_t)n * kMaskWords * 2);  // 32 bits to a double: exact
  for (size_t k = 0; k < (size_t)n * kMaskWords; k++)
    halves[2 * k] = (double)(uint32_t)words[k], halves[2 * k + 1] = (double)(uint32_t)(words[k] >> 32);
  g_out.add("I.mask_halves", halves.data(), (int64_t)halves.size());
}

// ---------------------------------------------------------------- X. pnp_epnp in the shape of k_pnp_hypotheses
// a job is (candidate, first index in X.idx, count); a candidate is (off, n) in i32 and K[4] in f64
__global__ void __launch_bounds__(kPnpLanes)
k_epnp(int n_jobs, const int* jobs, const int* cand_i, const double* cand_K, const float* Xw, const float* uv,
       const int* idx, double* o_Rt) {
  __shared__ double sA[144 * kPnpLanes], sV[144 * kPnpLanes];
  const int lane = threadIdx.x, job = blockIdx.x * kPnpLanes + lane;
  if (job >= n_jobs) return;
  const int c = jobs[job * 3];
  const PnpCandDev C = cand_of(cand_K + c * 4, cand_i[c * 2], cand_i[c * 2 + 1]);
  double R[3][3], t[3];
  pnp_epnp(C, Xw, uv, idx + jobs[job * 3 + 1], jobs[job * 3 + 2], sA, sV, lane, R, t);
  pnp_store_pose(R, t, o_Rt + 12 * (size_t)job);
}

static void run_epnp() {
  g_family = "X.pnp_epnp";
  int n_jobs, n_c, n_c2, np, np2, n_idx;
  const int* jobs_h = host_in<int32_t>("X.job", 3, &n_jobs);
  const int* cand_h = host_in<int32_t>("X.cand", 2, &n_c);
  const double* cand_K = dev_in<double>("X.cand_K", 4, &n_c2);
  same_n("X.cand_K", n_c, n_c2);
  const float* Xw = dev_in_float("X.Xw", 3, &np);
  const float* uv = dev_in_float("X.uv", 2, &np2);
  same_n("X.uv", np, np2);
  const int* idx_h = host_in<int32_t>("X.idx", 1, &n_idx);
  if (n_jobs > kMaxCases) die("more than 4096 jobs in", "X.job");
  for (int c = 0; c < n_c; c++)
    if (cand_h[c * 2] < 0 || cand_h[c * 2 + 1] < 0 || cand_h[c * 2] + cand_h[c * 2 + 1] > np) die("candidate outside the points", "X.cand");
  for (int j = 0; j < n_jobs; j++) {
    const int c = jobs_h[j * 3], first = jobs_h[j * 3 + 1], cnt = jobs_h[j * 3 + 2];
    if (c < 0 || c >= n_c || first < 0 || cnt < 4 || first + cnt > n_idx) die("job outside its tables", "X.job");
    for (int k = 0; k < cnt; k++)
      if (idx_h[first + k] < 0 || idx_h[first + k] >= cand_h[c * 2 + 1]) die("index outside the candidate", "X.idx");
  }
  const int* jobs = to_dev(jobs_h, (size_t)n_jobs * 3);
  const int* cand_i = to_dev(cand_h, (size_t)n_c * 2);
  const int* idx = to_dev(idx_h, (size_t)n_idx);
  const int blocks = n_jobs > 0 ? (n_jobs + kPnpLanes - 1) / kPnpLanes : 1;
  double* o_Rt = dev_out("X.Rt", (int64_t)n_jobs * 12);
  double* o_tap = dev_out("X.tap", (int64_t)blocks * kPnpLanes * kTapSlots);  // whole workgroups: a lane's slots exist
  CK(hipMemcpyToSymbol(HIP_SYMBOL(g_pnp_tap), &o_tap, sizeof(o_tap)));
  hipLaunchKernelGGL(k_epnp, dim3(blocks), dim3(kPnpLanes), 0, 0, n_jobs, jobs, cand_i, cand_K, Xw, uv, idx, o_Rt);
  finish_family();
}

// ---------------------------------------------------------------- T. s3s_top_eigenvector, H. s3s_horn, S. s3s_pose
__global__ void k_sim3(int n_t, const double* N, double* o_q, int n_h, const double* P1, const double* P2, const int* fix,
                       double* o_horn, int n_s, const double* Rts, double* o_pose) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_t) {
    double M[4][4], q[4];
    for (int r = 0; r < 4; r++)
      for (int c = 0; c < 4; c++) M[r][c] = N[i * 16 + r * 4 + c];
    s3s_top_eigenvector(M, q);
    for (int k = 0; k < 4; k++) o_q[i * 4 + k] = q[k];
  }
  if (i < n_h) {
    double A[3][3], B[3][3], R[3][3], t[3], s;
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) A[r][c] = P1[i * 9 + r * 3 + c], B[r][c] = P2[i * 9 + r * 3 + c];
    s3s_horn(A, B, fix[i] != 0, R, t, s);
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) o_horn[i * 13 + r * 3 + c] = R[r][c];
      o_horn[i * 13 + 9 + r] = t[r];
    }
    o_horn[i * 13 + 12] = s;
  }
  if (i < n_s) {
    double R[3][3], t[3];
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) R[r][c] = Rts[i * 13 + r * 3 + c];
      t[r] = Rts[i * 13 + 9 + r];
    }
    Sim3Pose T;
    s3s_pose(R, t, Rts[i * 13 + 12], T);
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) o_pose[i * 24 + r * 3 + c] = T.A12[r][c], o_pose[i * 24 + 12 + r * 3 + c] = T.A21[r][c];
      o_pose[i * 24 + 9 + r] = T.t12[r], o_pose[i * 24 + 21 + r] = T.t21[r];
    }
  }
}

static void run_sim3() {
  g_family = "T/H/S.sim3";
  int n_t, n_h, n_h2, n_h3, n_s;
  const double* N = dev_in<double>("T.N", 16, &n_t);
  const double* P1 = dev_in<double>("H.P1", 9, &n_h);
  const double* P2 = dev_in<double>("H.P2", 9, &n_h2);
  const int* fix = dev_in<int32_t>("H.fix_scale", 1, &n_h3);
  same_n("H.P2", n_h, n_h2), same_n("H.fix_scale", n_h, n_h3);
  const double* Rts = dev_in<double>("S.Rts", 13, &n_s);
  double* o_q = dev_out("T.s3s_top_eigenvector", n_t * 4);
  double* o_horn = dev_out("H.s3s_horn", n_h * 13);
  double* o_pose = dev_out("S.s3s_pose", n_s * 24);
  int n = n_t > n_h ? n_t : n_h;
  n = n_s > n ? n_s : n;
  hipLaunchKernelGGL(k_sim3, dim3(blocks_of(n)), dim3(64), 0, 0, n_t, N, o_q, n_h, P1, P2, fix, o_horn, n_s, Rts, o_pose);
  finish_family();
}

// ---------------------------------------------------------------- V. s3s_project, D. s3s_dist2, N. s3s_is_inlier
// a pose is A12[9], t12[3], A21[9], t21[3]
__global__ void k_views(const CamD* cams, int n_v, const int* vc, const double* vA, const float* vX, double* o_uv, int n_d,
                        const float* ab, double* o_d, int n_i, const int* ic, const double* iT, const float* iX,
                        const float* ime, double* o_in) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_v) {
    double A[3][3], t[3];
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) A[r][c] = vA[i * 12 + r * 3 + c];
      t[r] = vA[i * 12 + 9 + r];
    }
    float uv[2];
    if (vc[i * 2 + 1])
      s3s_project(cams[vc[i * 2]], A, t, vX + i * 3, uv);
    else
      s3s_project(cams[vc[i * 2]], nullptr, nullptr, vX + i * 3, uv);
    o_uv[i * 2] = uv[0], o_uv[i * 2 + 1] = uv[1];
  }
  if (i < n_d) o_d[i] = s3s_dist2(ab + i * 4, ab + i * 4 + 2);
  if (i < n_i) {
    Sim3Pose T;
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) T.A12[r][c] = iT[i * 24 + r * 3 + c], T.A21[r][c] = iT[i * 24 + 12 + r * 3 + c];
      T.t12[r] = iT[i * 24 + 9 + r], T.t21[r] = iT[i * 24 + 21 + r];
    }
    o_in[i] = s3s_is_inlier(T, cams[ic[i * 2]], cams[ic[i * 2 + 1]], iX + i * 6, iX + i * 6 + 3, ime[i * 2], ime[i * 2 + 1]) ? 1. : 0.;
  }
}

static void run_views() {
  g_family = "V/D/N.views";
  int64_t cf, ci;
  const double* hf = (const double*)g_in.find("C.cam_f64", 0, &cf);
  const int32_t* hi = (const int32_t*)g_in.find("C.cam_i32", 1, &ci);
  if (cf % 25 || ci % 2 || cf / 25 != ci / 2 || cf / 25 > 64) die("camera table", "C.cam_f64 / C.cam_i32");
  const int n_cams = (int)(cf / 25);
  std::vector<CamD> hc(n_cams ? n_cams : 1);
  for (int c = 0; c < n_cams; c++) {  // (fx, fy, cx, cy, bf, Rcb[9], tcb[3], k[8]) in f64, (model, num_k) in i32
    const double* f = hf + c * 25;
    CamD& d = hc[c];
    d.fx = f[0], d.fy = f[1], d.cx = f[2], d.cy = f[3], d.bf = f[4];
    for (int k = 0; k < 9; k++) d.Rcb[k] = f[5 + k];
    for (int k = 0; k < 3; k++) d.tcb[k] = f[14 + k];
    for (int k = 0; k < 8; k++) d.k[k] = f[17 + k];
    d.model = hi[c * 2], d.num_k = hi[c * 2 + 1];
    if (d.model < 0 || d.model > 2 || (d.model == 1 && (d.num_k < 2 || d.num_k > 6))) die("camera model", "C.cam_i32");
  }
  const CamD* cams = to_dev(hc.data(), hc.size());
  int n_v, n_v2, n_v3, n_d, n_i, n_i2, n_i3, n_i4;
  const int* vc_h = host_in<int32_t>("V.cam", 2, &n_v);
  const double* vA = dev_in<double>("V.A", 12, &n_v2);
  const float* vX = dev_in_float("V.X", 3, &n_v3);
  same_n("V.A", n_v, n_v2), same_n("V.X", n_v, n_v3);
  const float* ab = dev_in_float("D.ab", 4, &n_d);
  const int* ic_h = host_in<int32_t>("N.cam", 2, &n_i);
  const double* iT = dev_in<double>("N.T", 24, &n_i2);
  const float* iX = dev_in_float("N.X", 6, &n_i3);
  const float* ime = dev_in_float("N.max_err", 2, &n_i4);
  same_n("N.T", n_i, n_i2), same_n("N.X", n_i, n_i3), same_n("N.max_err", n_i, n_i4);
  if (n_v > kMaxCases || n_i > kMaxCases) die("more than 4096 cases in", "V.cam / N.cam");
  for (int i = 0; i < n_v; i++)
    if (vc_h[i * 2] < 0 || vc_h[i * 2] >= n_cams) die("camera index out of range in", "V.cam");
  for (int i = 0; i < n_i * 2; i++)
    if (ic_h[i] < 0 || ic_h[i] >= n_cams) die("camera index out of range in", "N.cam");
  const int* vc = to_dev(vc_h, (size_t)n_v * 2);
  const int* ic = to_dev(ic_h, (size_t)n_i * 2);
  double* o_uv = dev_out("V.s3s_project", n_v * 2);
  double* o_d = dev_out("D.s3s_dist2", n_d);
  double* o_in = dev_out("N.s3s_is_inlier", n_i);
  int n = n_v > n_d ? n_v : n_d;
  n = n_i > n ? n_i : n;
  hipLaunchKernelGGL(k_views, dim3(blocks_of(n)), dim3(64), 0, 0, cams, n_v, vc, vA, vX, o_uv, n_d, ab, o_d, n_i, ic, iT, iX,
                     ime, o_in);
  finish_family();
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: solver_algebra_test in.bin out.bin\n");
    return 2;
  }
  g_in.load(argv[1]);
  g_family = "L.lstsq6<3>";
  run_lstsq<3>("L.A3", "L.b3", "L.pnp_lstsq6<3>");
  g_family = "L.lstsq6<4>";
  run_lstsq<4>("L.A4", "L.b4", "L.pnp_lstsq6<4>");
  g_family = "L.lstsq6<5>";
  run_lstsq<5>("L.A5", "L.b5", "L.pnp_lstsq6<5>");
  run_small();
  run_points();
  run_check();
  run_epnp();
  run_sim3();
  run_views();
  g_out.write(argv[2]);
  return 0;
}
