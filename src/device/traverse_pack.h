// Compact tree for the score update by traversal over packed rows (traverse_kernels.h).
//
// One tree is staged as four 256-byte aligned parts in one upload (CompactLayout): the nodes,
// the categorical node data, the leaf values and the categorical words. PackCompactNode turns a
// numerical node into the group-bin predicate that traverse_kernels.h describes (lo / hi / tg /
// gmiss / out_left); categorical nodes keep the decode + bitset path (TCat).
// Free of HIP headers: plain C++ translation units include it.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "lgap/dataset.h"
#include "lgap/log.h"
#include "lgap/tree.h"

namespace lgap {
namespace device {

struct TNode {
  uint16_t group, lo, hi, tg;
  int16_t gmiss;   // -1: no separate missing bin in range
  uint8_t flags;   // bit0 out_left, bit1 default_left, bit2 categorical
  uint8_t pad;
  int16_t left, right;  // >= 0: node, < 0: ~leaf
};
static_assert(sizeof(TNode) == 16, "TNode layout");

// categorical node data, indexed by node (meaningful for categorical nodes only)
struct TCat {
  int offset, num_bin, mfb, begin, nwords, pad;
};

constexpr uint8_t kTOutLeft = 1, kTDefaultLeft = 2, kTCat = 4;

inline size_t Round256(size_t x) { return (x + 255) & ~static_cast<size_t>(255); }

// offsets of the categorical node data, the leaf values and the categorical words (the nodes
// sit at 0)
struct CompactLayout {
  size_t cat, leaf, bit, total;
};
inline CompactLayout CompactTreeLayout(const Tree* tree) {
  const int nn = tree->num_leaves() - 1, nl = tree->num_leaves();
  const size_t node_bytes = Round256(sizeof(TNode) * nn), cat_bytes = Round256(sizeof(TCat) * nn);
  const size_t leaf_bytes = Round256(sizeof(double) * nl);
  const size_t bit_bytes = sizeof(uint32_t) * std::max<size_t>(1, tree->cat_threshold_inner().size());
  CompactLayout z;
  z.cat = node_bytes;
  z.leaf = z.cat + cat_bytes;
  z.bit = z.leaf + leaf_bytes;
  z.total = z.bit + bit_bytes;
  return z;
}

// One node of feature `fi`: decision type `dt` (lgap/tree.h), threshold_in_bin `thr` (numerical
// nodes), children, and a categorical node's words [cat_begin, cat_begin + cat_nwords) of the
// tree's inner bitsets. *c is written for categorical nodes only.
inline void PackCompactNode(const FeatureInfo& fi, int8_t dt, int thr, int left, int right, int cat_begin,
                            int cat_nwords, TNode* node, TCat* c) {
  const int missing = Tree::GetMissingType(dt);
  const bool dleft = Tree::GetDecisionType(dt, kDefaultLeftMask);
  const int offset = fi.offset, nb = fi.num_bin, mfb = static_cast<int>(fi.mfb);
  TNode& d = *node;
  std::memset(&d, 0, sizeof(d));
  d.group = static_cast<uint16_t>(fi.group);
  d.left = static_cast<int16_t>(left);
  d.right = static_cast<int16_t>(right);
  d.gmiss = -1;
  if (Tree::GetDecisionType(dt, kCategoricalMask)) {
    d.flags = kTCat;
    *c = {offset, nb, mfb, cat_begin, cat_nwords, 0};
    return;
  }
  const int bmiss = missing == 1 ? static_cast<int>(fi.default_bin) : (missing == 2 ? nb - 1 : -1);
  // stored feature bins k = 0 .. nb - 2 sit at group bins offset + k (the mfb is implicit)
  d.lo = static_cast<uint16_t>(offset);
  d.hi = static_cast<uint16_t>(offset + nb - 2);
  const bool out_left = bmiss == mfb ? dleft : (mfb <= thr);
  if (bmiss >= 0 && bmiss != mfb) d.gmiss = static_cast<int16_t>(offset + (bmiss < mfb ? bmiss : bmiss - 1));
  // last group bin whose feature bin is <= thr; below `offset` (thr == mfb == 0) no stored bin
  // goes left, and tg = 0 makes `gb <= tg` false for every in-range bin (offset >= 1)
  const int tg = offset + (thr < mfb ? thr : thr - 1);
  d.tg = static_cast<uint16_t>(tg < offset ? 0 : tg);
  d.flags = static_cast<uint8_t>((out_left ? kTOutLeft : 0) | (dleft ? kTDefaultLeft : 0));
}

// `tree` (at least two leaves) into the z.total bytes at hp
inline void PackCompactTree(const Tree* tree, const Dataset* data, char* hp, const CompactLayout& z) {
  const int nn = tree->num_leaves() - 1, nl = tree->num_leaves();
  LGAP_CHECK(nn <= 32767);  // (children are int16_t)
  const auto& cb = tree->cat_boundaries_inner();
  const auto& ct = tree->cat_threshold_inner();
  TNode* nodes = reinterpret_cast<TNode*>(hp);
  TCat* cats = reinterpret_cast<TCat*>(hp + z.cat);
  for (int i = 0; i < nn; ++i) {
    const int8_t dt = tree->decision_type(i);
    const int thr = static_cast<int>(tree->threshold_in_bin(i));
    const bool cat = Tree::GetDecisionType(dt, kCategoricalMask);
    PackCompactNode(data->feature(tree->split_feature_inner(i)), dt, thr, tree->left_child(i), tree->right_child(i),
                    cat ? cb[thr] : 0, cat ? cb[thr + 1] - cb[thr] : 0, &nodes[i], &cats[i]);
  }
  double* lv = reinterpret_cast<double*>(hp + z.leaf);
  for (int l = 0; l < nl; ++l) lv[l] = tree->LeafOutput(l);
  uint32_t* cw = reinterpret_cast<uint32_t*>(hp + z.bit);
  for (size_t i = 0; i < ct.size(); ++i) cw[i] = ct[i];
}

// the packed tree as the launch wrappers of traverse_kernels.h take it
struct CompactTreeDev {
  const TNode* nodes;
  const TCat* cats;
  const uint32_t* cat_bits;
  const double* leaf_value;
  int num_nodes, num_leaves;
};
// base: the device copy of what PackCompactTree wrote for a tree of num_leaves leaves
inline CompactTreeDev CompactTreeAt(const char* base, const CompactLayout& z, int num_leaves) {
  return {reinterpret_cast<const TNode*>(base), reinterpret_cast<const TCat*>(base + z.cat),
          reinterpret_cast<const uint32_t*>(base + z.bit), reinterpret_cast<const double*>(base + z.leaf),
          num_leaves - 1, num_leaves};
}

}  // namespace device
}  // namespace lgap
