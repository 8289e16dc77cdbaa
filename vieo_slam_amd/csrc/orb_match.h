// orb_match.h -- what every ORBmatcher search does with one pair of keys, once: the thresholds (ORBmatcher.cc:20-22),
// DescriptorDistance (:1645-1667; xor + popcount on the 8 dwords of a 32-byte row, v_bcnt_u32_b32 on the device), the
// rotation bin of a pair (e.g. :1453-1460) and ComputeThreeMaxima (:1608-1641) as the mask of the bins it erases.
// Host and device: the kernels of seven files inline the distance and the bin, the host walks of bow_walk.h and
// tri_search.hip call the bin and the maxima, g++ compiles the header on its own (tests/emul/bow_walk_emul.cc).  The
// three assignment kernels of proj_search.hip keep their own statement of the maxima over the LDS histogram: through
// this function their machine code came out in another order (profiles/orb_match_common.md).
#pragma once
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define VIEO_OM_HD __host__ __device__ __forceinline__
#else
#define VIEO_OM_HD static inline
namespace vieo {
struct uint4 { uint32_t x, y, z, w; };
}  // namespace vieo
#endif

namespace vieo {

static const int kThHigh = 100, kThLow = 50, kHistoLen = 30;  // TH_HIGH, TH_LOW, HISTO_LENGTH

// both descriptors in registers
VIEO_OM_HD int hamming256(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
  return __builtin_popcount(a0.x ^ b0.x) + __builtin_popcount(a0.y ^ b0.y) + __builtin_popcount(a0.z ^ b0.z) +
         __builtin_popcount(a0.w ^ b0.w) + __builtin_popcount(a1.x ^ b1.x) + __builtin_popcount(a1.y ^ b1.y) +
         __builtin_popcount(a1.z ^ b1.z) + __builtin_popcount(a1.w ^ b1.w);
}
// b, a: 32 bytes, 16-byte aligned
VIEO_OM_HD int hamming256(const uint4 a0, const uint4 a1, const void* b) {
  return hamming256(a0, a1, ((const uint4*)b)[0], ((const uint4*)b)[1]);
}
VIEO_OM_HD int hamming256(const void* a, const void* b) { return hamming256(((const uint4*)a)[0], ((const uint4*)a)[1], b); }

// the bin of a pair's rotation; 0 .. kHistoLen - 1 for angles in [0, 360), not checked here
VIEO_OM_HD int rot_bin(float angle1, float angle2) {
  float rot = angle1 - angle2;
  if (rot < 0.0f) rot += 360.0f;
  int bin = (int)roundf(rot * (1.0f / kHistoLen));
  if (bin == kHistoLen) bin = 0;
  return bin;
}

// ComputeThreeMaxima over the kHistoLen counts, as the mask of the bins whose matches are erased: every bin but the
// up to three it keeps (the indices stay -1 when every count is 0: all bins)
VIEO_OM_HD unsigned three_maxima(const int* hist) {
  int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
  for (int i = 0; i < kHistoLen; i++) {
    const int s = hist[i];
    if (s > max1)
      max3 = max2, max2 = max1, max1 = s, ind3 = ind2, ind2 = ind1, ind1 = i;
    else if (s > max2)
      max3 = max2, max2 = s, ind3 = ind2, ind2 = i;
    else if (s > max3)
      max3 = s, ind3 = i;
  }
  if (max2 < 0.1f * (float)max1)
    ind2 = -1, ind3 = -1;
  else if (max3 < 0.1f * (float)max1)
    ind3 = -1;
  unsigned losers = (1u << kHistoLen) - 1u;
  if (ind1 >= 0) losers &= ~(1u << ind1);
  if (ind2 >= 0) losers &= ~(1u << ind2);
  if (ind3 >= 0) losers &= ~(1u << ind3);
  return losers;
}

}  // namespace vieo
