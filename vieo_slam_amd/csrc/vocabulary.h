// vocabulary.h -- the resident vocabulary tree as bow_transform.hip and kf_database.hip see it.
#pragma once
#include "common.h"

namespace vieo {

// Device order: breadth first from the root (device index 0), so that a node's children are ONE contiguous run in child
// order: the k child descriptors of a level are one 32 k byte read.
struct VocNode {
  int32_t child_first, child_count;  // device index of the first child; 0 children = a word
  int32_t word_id;                   // -1: an inner node
  uint32_t node_id;                  // the id of the file (what mFeatVec reports)
  double weight;
};  // 24 bytes

}  // namespace vieo

struct vieo_vocabulary {
  int k = 0, L = 0, n_nodes = 0, n_words = 0, dev = 0;
  vieo::VocNode* d_nodes = nullptr;  // [n_nodes + 1]
  uint8_t* d_desc = nullptr;         // [n_nodes + 1][32] in device order (the root's: zero, never read)
};
