// ORBmatcher_init_hot.cc -- replacement DEFINITION of the matcher of the monocular initialisation, on top of the C-ABI of
// libvieo_hot.so.  Compiled inside the reference tree against the reference's own include/ORBmatcher.h beside
// ORBmatcher_hot.cc; the member is compiled out of src/ORBmatcher.cc.
// Tracking::MonocularInitialization calls it unchanged.
//
//   int SearchForInitialization(Frame&, Frame&, vbPrevMatched, vnMatches12, windowSize)  ORBmatcher.cc:628-723
//
// Nothing of the caller's objects is written but the two vectors the reference writes.  No CPU fallback: a failing C-ABI
// call aborts like the reference's CV_Assert.
#include "ORBmatcher.h"

#include <cstdio>
#include <cstdlib>

#include "vieo_flatten.hpp"

namespace VIEO_SLAM {

namespace {

static_assert(sizeof(cv::KeyPoint) == sizeof(vieo_keypoint), "cv::KeyPoint layout (28 bytes) is the C-ABI's");
static_assert(sizeof(cv::Point2f) == 2 * sizeof(float) && sizeof(int) == sizeof(int32_t),
              "vbPrevMatched / vnMatches12 as the C-ABI reads them");

[[noreturn]] void hot_fail(const char* what, int rc) {
  std::fprintf(stderr, "vieo_hot: %s failed (%d): %s\n", what, rc, vieo_last_error());
  std::abort();  // the reference's error convention for programming errors (CV_Assert)
}

}  // namespace

int ORBmatcher::SearchForInitialization(Frame& F1, Frame& F2, vector<cv::Point2f>& vbPrevMatched, vector<int>& vnMatches12,
                                        int windowSize) {
  const size_t n1 = F1.mvKeysUn.size(), n2 = F2.mvKeysUn.size();
  vnMatches12 = vector<int>(n1, -1);
  // (no grid yet: GetFeaturesInArea returns nothing, FrameBase.cpp:98)
  if (n1 == 0 || vieo_shim::GridAccess::bounds().empty()) return 0;
  if (vbPrevMatched.size() < n1) hot_fail("SearchForInitialization: vbPrevMatched is shorter than F1.mvKeysUn", VIEO_E_INVALID);
  vieo_init_pair P;
  std::memset(&P, 0, sizeof(P));
  P.keys1 = reinterpret_cast<const vieo_keypoint*>(F1.mvKeysUn.data()), P.desc1 = F1.mDescriptors.ptr<unsigned char>(0);
  P.keys2 = reinterpret_cast<const vieo_keypoint*>(F2.mvKeysUn.data());
  P.desc2 = n2 ? F2.mDescriptors.ptr<unsigned char>(0) : nullptr;
  P.prev_matched = &vbPrevMatched[0].x, P.matches12 = vnMatches12.data();
  P.n1 = (int32_t)n1, P.n2 = (int32_t)n2, P.window_size = windowSize;
  const int rc = vieo_search_for_initialization(&P, 1, vieo_shim::GridAccess::bounds()[0].data(), mfNNratio, mbCheckOrientation ? 1 : 0);
  if (rc != VIEO_OK) hot_fail("vieo_search_for_initialization", rc);
  return P.n_matches;
}

}  // namespace VIEO_SLAM
