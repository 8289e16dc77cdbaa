// Runs shim/OdomPreIntegrator_hot.cc -- the drop-in IMUPreIntegratorBase<IMUDataBase>::PreIntegration -- the way the
// reference's tracking calls it (tests/test_shim_compile.py writes the input, compares the output with the oracle):
// one aligned_list<IMUDataBase>, a breset = true call from a key frame's time (Tracking.h:417 breset_intkf on the
// first frame behind it), then breset = false continuations over [t_{k-1}, t_k] on the same pre-integrator
// (Frame::PreIntegrationFromLastKF, src/Frame.cc:60-67).  Built against the mock headers of tests/shim_compile/mock,
// linked with libvieo_hot.so.
//
//   preint_driver IN OUT
//   IN  (float64): K, K x (t, w[3], a[3]), sigma_g[9], sigma_a[9] (row-major), freq_ref, dt_cov_noise_fixed,
//                  n_calls, n_calls x (ti, tj, i0, i1, breset, bg[3], ba[3]) -- the call passes the list's [i0, i1)
//   OUT (float64): per call the return value, mdeltatij, mRij, mvij, mpij, mJgRij, mJgvij, mJavij, mJgpij, mJapij,
//                  mSigmaij, mSigmaijPRV (row-major), after the call
//   exit 0 done, 1 bad input, 2 no gfx950 device
#include <cstdio>
#include <iterator>
#include <vector>

#include "Frame.h"
#include "vieo_hot.h"

namespace VIEO_SLAM {
Eigen::Matrix3d IMUDataBase::mSigmag, IMUDataBase::mSigmaa;
double IMUDataBase::mInvSigmabg2 = 0, IMUDataBase::mInvSigmaba2 = 0;
int IMUDataBase::mdt_cov_noise_fixed = 0;
double IMUDataBase::mFreqRef = 0;
}  // namespace VIEO_SLAM

using namespace VIEO_SLAM;

namespace {
template <int R, int C>
void put(std::vector<double>& o, const Eigen::Matrix<double, R, C>& m) {
  for (int r = 0; r < R; ++r)
    for (int c = 0; c < C; ++c) o.push_back(m(r, c));
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: preint_driver IN OUT\n");
    return 1;
  }
  if (!vieo_device_available()) {
    std::fprintf(stderr, "no gfx950 device: %s (there is no CPU fallback)\n", vieo_last_error());
    return 2;
  }
  std::vector<double> in;
  {
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 1;
    double v;
    while (std::fread(&v, sizeof v, 1, f) == 1) in.push_back(v);
    std::fclose(f);
  }
  size_t at = 0;
  auto next = [&]() { return at < in.size() ? in[at++] : 0.0; };
  const int K = (int)next();
  aligned_list<IMUDataBase> imu;
  for (int k = 0; k < K; ++k) {
    IMUDataBase s;
    s.mtm = next();
    for (int r = 0; r < 3; ++r) s.mw(r) = next();
    for (int r = 0; r < 3; ++r) s.ma(r) = next();
    imu.push_back(s);
  }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) IMUDataBase::mSigmag(r, c) = next();
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) IMUDataBase::mSigmaa(r, c) = next();
  IMUDataBase::mFreqRef = next();
  IMUDataBase::mdt_cov_noise_fixed = (int)next();
  const int n_calls = (int)next();
  if (K <= 0 || n_calls <= 0 || in.size() != at + 11 * (size_t)n_calls) {
    std::fprintf(stderr, "preint_driver: malformed input\n");
    return 1;
  }
  IMUPreintegrator pre;  // (every member is written by the first call, a breset = true one)
  pre.mdeltatij = 0;
  std::vector<double> out;
  for (int c = 0; c < n_calls; ++c) {
    const double ti = next(), tj = next();
    const int i0 = (int)next(), i1 = (int)next();
    const bool breset = next() != 0;
    Eigen::Vector3d bg, ba;
    for (int r = 0; r < 3; ++r) bg(r) = next();
    for (int r = 0; r < 3; ++r) ba(r) = next();
    if (i0 < 0 || i0 > i1 || i1 > K) return 1;
    const aligned_list<IMUDataBase>::const_iterator b = std::next(imu.cbegin(), i0), e = std::next(imu.cbegin(), i1);
    const int ret = pre.PreIntegration(ti, tj, bg, ba, b, e, breset);
    out.push_back(ret);
    out.push_back(pre.mdeltatij);
    put(out, pre.mRij), put(out, pre.mvij), put(out, pre.mpij);
    put(out, pre.mJgRij), put(out, pre.mJgvij), put(out, pre.mJavij), put(out, pre.mJgpij), put(out, pre.mJapij);
    put(out, pre.mSigmaij), put(out, pre.mSigmaijPRV);
  }
  FILE* f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 1;
  std::fclose(f);
  std::printf("preint_driver ok: %d calls\n", n_calls);
  return 0;
}
