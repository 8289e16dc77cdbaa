// vocabulary.hip -- the DBoW2 vocabulary handle (reference loop/DBoW2/DBoW2/TemplatedVocabulary.h): built from a flat
// node table or from the reference's text / binary files, validated, re-laid breadth first (vocabulary.h) and uploaded
// once.  Host code only; the kernels that read the tree are in bow_transform.hip.
#include <cerrno>
#include <cstdlib>
#include <string>
#include <vector>

#include "vocabulary.h"

namespace vieo {

static int voc_header_ok(int k, int L, int scoring, int weighting) {
  if (k < 0 || k > 20 || L < 1 || L > 10) {
    set_error("vocabulary: k = %d, L = %d outside 0..20, 1..10", k, L);
    return VIEO_E_INVALID;
  }
  if (scoring != 0 || weighting != 0) {
    set_error("vocabulary: scoring %d / weighting %d: only L1_NORM (0) with TF_IDF (0) is supported", scoring, weighting);
    return VIEO_E_INVALID;
  }
  return VIEO_OK;
}

static int voc_build(vieo_vocabulary** out, int k, int L, int scoring, int weighting, const vieo_voc_node* nodes, int n) {
  if (!out || n < 0 || (n > 0 && !nodes)) return VIEO_E_INVALID;
  int rc = voc_header_ok(k, L, scoring, weighting);
  if (rc != VIEO_OK) return rc;
  std::vector<int> first(n + 2, 0);  // children of node p: kids[first[p] .. first[p + 1]), in row order
  for (int i = 0; i < n; i++) {
    const int p = nodes[i].parent;
    if (p < 0 || p >= i + 1) {
      set_error("vocabulary: node %d has parent %d", i + 1, p);
      return VIEO_E_INVALID;
    }
    first[p + 1]++;
  }
  for (int id = 0; id <= n; id++) {
    const int c = first[id + 1];
    const bool leaf = id > 0 && nodes[id - 1].is_leaf != 0;
    if (c > k || (id > 0 && leaf != (c == 0))) {
      set_error("vocabulary: node %d (%s) has %d children, k = %d", id, leaf ? "a leaf" : "inner", c, k);
      return VIEO_E_INVALID;
    }
  }
  for (int id = 0; id <= n; id++) first[id + 1] += first[id];
  std::vector<int> kids(n), fill(first.begin(), first.end() - 1);
  for (int i = 0; i < n; i++) kids[fill[nodes[i].parent]++] = i + 1;
  std::vector<int> word(n + 1, -1);
  int n_words = 0;
  for (int i = 0; i < n; i++)
    if (nodes[i].is_leaf) word[i + 1] = n_words++;
  // breadth first: a node's children get consecutive device indices
  std::vector<int> order;
  order.reserve(n + 1);
  order.push_back(0);
  std::vector<VocNode> dn(n + 1);
  std::vector<uint8_t> dd((size_t)(n + 1) * 32, 0);
  for (size_t q = 0; q < order.size(); q++) {
    const int id = order[q];
    VocNode& N = dn[q];
    N.child_first = (int)order.size(), N.child_count = first[id + 1] - first[id];
    N.word_id = word[id], N.node_id = (uint32_t)id;
    N.weight = id ? nodes[id - 1].weight : 0.0;
    if (id) memcpy(&dd[q * 32], nodes[id - 1].descriptor, 32);
    for (int c = first[id]; c < first[id + 1]; c++) order.push_back(kids[c]);
  }
  if ((int)order.size() != n + 1) {  // (cannot happen: every parent chain ends at the root)
    set_error("vocabulary: %d of %d nodes hang on the root", (int)order.size() - 1, n);
    return VIEO_E_INVALID;
  }
  if ((rc = require_device()) != VIEO_OK) return rc;
  vieo_vocabulary* V = new vieo_vocabulary;
  V->k = k, V->L = L, V->n_nodes = n, V->n_words = n_words;
  (void)hipGetDevice(&V->dev);
  hipError_t e = hipMalloc((void**)&V->d_nodes, dn.size() * sizeof(VocNode));
  if (e == hipSuccess) e = hipMalloc((void**)&V->d_desc, dd.size());
  if (e == hipSuccess) e = hipMemcpy(V->d_nodes, dn.data(), dn.size() * sizeof(VocNode), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(V->d_desc, dd.data(), dd.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    set_error("vocabulary: upload of %d nodes -> %s", n, hipGetErrorString(e));
    vieo_vocabulary_destroy(V);
    return VIEO_E_HIP;
  }
  *out = V;
  return VIEO_OK;
}

static bool read_file(const char* path, std::string& data) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  char buf[1 << 16];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), f)) > 0) data.append(buf, got);
  const bool ok = !ferror(f);
  fclose(f);
  return ok;
}

// "k L scoring weighting", then per node "parent is_leaf d0 .. d31 weight"; empty lines are skipped
static int voc_parse_text(const std::string& s, int hdr[4], std::vector<vieo_voc_node>& nodes) {
  const char* p = s.c_str();
  const char* end = p + s.size();
  auto line_end = [&](const char* q) {
    while (q < end && *q != '\n') q++;
    return q;
  };
  auto blank = [](const char* a, const char* b) {
    for (; a < b; a++)
      if (*a != ' ' && *a != '\t' && *a != '\r') return false;
    return true;
  };
  const char* le = line_end(p);
  {
    std::string h(p, le);
    char* q = &h[0];
    for (int i = 0; i < 4; i++) {
      char* r;
      errno = 0;
      const long v = strtol(q, &r, 10);
      if (r == q || errno || v < -1000 || v > 1000) return VIEO_E_INVALID;
      hdr[i] = (int)v, q = r;
    }
  }
  for (p = le < end ? le + 1 : end; p < end; p = le < end ? le + 1 : end) {
    le = line_end(p);
    if (blank(p, le)) continue;
    std::string l(p, le);
    char* q = &l[0];
    char* r;
    vieo_voc_node N;
    long v[34];
    for (int i = 0; i < 34; i++) {
      errno = 0;
      v[i] = strtol(q, &r, 10);
      if (r == q || errno || (i >= 2 && (v[i] < 0 || v[i] > 255))) return VIEO_E_INVALID;
      q = r;
    }
    if (v[0] < INT32_MIN || v[0] > INT32_MAX) return VIEO_E_INVALID;
    N.parent = (int32_t)v[0], N.is_leaf = v[1] > 0;
    for (int i = 0; i < 32; i++) N.descriptor[i] = (uint8_t)v[2 + i];
    N.weight = strtod(q, &r);
    if (r == q) return VIEO_E_INVALID;
    nodes.push_back(N);
  }
  return VIEO_OK;
}

static int voc_parse_binary(const std::string& s, int hdr[4], std::vector<vieo_voc_node>& nodes) {
  if (s.size() < 24) return VIEO_E_INVALID;
  uint32_t nb_nodes, size_node;
  memcpy(&nb_nodes, &s[0], 4), memcpy(&size_node, &s[4], 4), memcpy(hdr, &s[8], 16);
  if (size_node != 41 || nb_nodes < 1) return VIEO_E_INVALID;
  if (voc_header_ok(hdr[0], hdr[1], 0, 0) != VIEO_OK) return VIEO_E_INVALID;
  if (hdr[0] > 1) {  // the reference's bound: at most 1 + k + .. + k^L nodes
    double full = 0, pw = 1;
    for (int l = 0; l <= hdr[1]; l++) full += pw, pw *= hdr[0];
    if ((double)nb_nodes > full) return VIEO_E_INVALID;
  }
  if ((s.size() - 24) / 41 < (size_t)nb_nodes - 1) return VIEO_E_INVALID;  // a short file
  nodes.resize(nb_nodes - 1);
  for (size_t i = 0; i + 1 < nb_nodes; i++) {
    const char* r = &s[24 + 41 * i];
    float w;
    memcpy(&nodes[i].parent, r, 4), memcpy(nodes[i].descriptor, r + 4, 32), memcpy(&w, r + 36, 4);
    nodes[i].weight = (double)w, nodes[i].is_leaf = r[40] != 0;
  }
  return VIEO_OK;
}

}  // namespace vieo

extern "C" int vieo_vocabulary_create(vieo_vocabulary** out, int k, int L, int scoring, int weighting,
                                      const vieo_voc_node* nodes, int n_nodes) {
  return vieo::voc_build(out, k, L, scoring, weighting, nodes, n_nodes);
}

extern "C" int vieo_vocabulary_load(vieo_vocabulary** out, const char* path) {
  using namespace vieo;
  if (!out || !path) return VIEO_E_INVALID;
  std::string data;
  if (!read_file(path, data)) {
    set_error("vocabulary: cannot read %s", path);
    return VIEO_E_INVALID;
  }
  int hdr[4] = {0, 0, 0, 0};
  std::vector<vieo_voc_node> nodes;
  const bool text = std::string(path).find(".txt") != std::string::npos;
  if ((text ? voc_parse_text(data, hdr, nodes) : voc_parse_binary(data, hdr, nodes)) != VIEO_OK) {
    set_error("vocabulary: %s is not a correct %s file", path, text ? "text" : "binary");
    return VIEO_E_INVALID;
  }
  return voc_build(out, hdr[0], hdr[1], hdr[2], hdr[3], nodes.data(), (int)nodes.size());
}

extern "C" int vieo_vocabulary_info(const vieo_vocabulary* voc, vieo_voc_info* info) {
  if (!voc || !info) return VIEO_E_INVALID;
  info->k = voc->k, info->L = voc->L, info->n_nodes = voc->n_nodes, info->n_words = voc->n_words;
  return VIEO_OK;
}

extern "C" void vieo_vocabulary_destroy(vieo_vocabulary* voc) {
  if (!voc) return;
  if (voc->d_nodes) (void)hipFree(voc->d_nodes);
  if (voc->d_desc) (void)hipFree(voc->d_desc);
  delete voc;
}
