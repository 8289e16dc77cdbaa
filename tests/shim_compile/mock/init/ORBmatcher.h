// TEST DOUBLE (see ../reference_decls.hpp) -- include/ORBmatcher.h as shim/ORBmatcher_init_hot.cc needs it: the class with
// SearchForInitialization, which ../reference_decls.hpp does not declare.  This directory goes in front of the mock
// directory on the include path of that one translation unit.  The shared stand-ins are taken as they are; their reduced
// ORBmatcher is given another name while they are read, and the class is declared here with the member, its signature as
// in the reference's include/ORBmatcher.h:74-75.  Declarations only; nothing is linked or run; no parity evidence.
#pragma once
#define ORBmatcher ORBmatcher_without_initialization
#include "../reference_decls.hpp"
#undef ORBmatcher

namespace VIEO_SLAM {

class ORBmatcher {
 public:
  static const int TH_LOW, TH_HIGH, HISTO_LENGTH;
  ORBmatcher(float nnratio = 0.6, bool checkOri = true);
  int SearchForInitialization(Frame &F1, Frame &F2, std::vector<cv::Point2f> &vbPrevMatched,
                              std::vector<int> &vnMatches12, int windowSize = 10);

 protected:
  float mfNNratio;
  bool mbCheckOrientation;
};

}  // namespace VIEO_SLAM
