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
#include <vector>

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

// ---- A forest: `count` compact trees in one upload, walked in list order by one pass over the
// rows (k_traverse_forest). Every tree is one contiguous blob, its nodes then its leaf values
// (a multiple of 16 bytes), so a RUN of consecutive trees is one contiguous byte range that the
// kernel copies into LDS with 16-byte loads. A run holds as many consecutive trees as fit
// kForestRunBytes (the budget's reasoning: the kernel's header comment); a tree larger than
// the budget is a run of its own whose nodes and leaves are read from global memory. A
// one-leaf tree has no nodes and one leaf value. Categorical node data is kept only for trees
// that have a categorical node; TCat::begin already includes the tree's offset into the
// forest's categorical words.
constexpr int kForestRunBytes = 20 * 1024;

struct TForestTree {
  uint32_t blob;  // byte offset of the tree's nodes in the blob part; its leaf values follow them
  int32_t cat;    // index of node 0's TCat (meaningful for trees with a categorical node)
  int32_t num_nodes, num_leaves;
};
static_assert(sizeof(TForestTree) == 16, "TForestTree layout");
struct TForestRun {
  int32_t first, count;  // trees [first, first + count)
  uint32_t begin, bytes;  // their blobs; bytes > kForestRunBytes: one tree, walked from global memory
};

inline size_t ForestTreeBytes(int num_leaves) {
  return sizeof(TNode) * static_cast<size_t>(num_leaves - 1) + ((sizeof(double) * num_leaves + 15) & ~static_cast<size_t>(15));
}

inline bool HasCategoricalNode(const Tree* tree) {
  for (int i = 0; i < tree->num_leaves() - 1; ++i) {
    if (Tree::GetDecisionType(tree->decision_type(i), kCategoricalMask)) return true;
  }
  return false;
}

// offsets of the run table, the blobs, the categorical node data and the categorical words
// (the tree table sits at 0)
struct ForestLayout {
  size_t run, blob, cat, bit, total;
  int num_trees;
  std::vector<TForestRun> runs;
};
inline ForestLayout CompactForestLayout(const Tree* const* trees, int count) {
  ForestLayout z;
  z.num_trees = count;
  size_t blob = 0, cats = 0, bits = 0;
  for (int i = 0; i < count; ++i) {
    const size_t b = ForestTreeBytes(trees[i]->num_leaves());
    if (z.runs.empty() || z.runs.back().bytes + b > static_cast<size_t>(kForestRunBytes)) {
      z.runs.push_back({i, 0, static_cast<uint32_t>(blob), 0u});
    }
    z.runs.back().count += 1;
    z.runs.back().bytes += static_cast<uint32_t>(b);
    blob += b;
    if (HasCategoricalNode(trees[i])) {
      cats += trees[i]->num_leaves() - 1;
      bits += trees[i]->cat_threshold_inner().size();
    }
  }
  z.run = Round256(sizeof(TForestTree) * std::max(count, 1));
  z.blob = z.run + Round256(sizeof(TForestRun) * std::max<size_t>(z.runs.size(), 1));
  z.cat = z.blob + Round256(std::max<size_t>(blob, 16));
  z.bit = z.cat + Round256(sizeof(TCat) * std::max<size_t>(cats, 1));
  z.total = z.bit + sizeof(uint32_t) * std::max<size_t>(bits, 1);
  return z;
}

// `trees` (each at most 32768 leaves) into the z.total bytes at hp. The leaf values are copied
// as they are now: the caller may rescale the trees afterwards.
inline void PackCompactForest(const Tree* const* trees, const Dataset* data, char* hp, const ForestLayout& z) {
  TForestTree* tt = reinterpret_cast<TForestTree*>(hp);
  std::memcpy(hp + z.run, z.runs.data(), sizeof(TForestRun) * z.runs.size());
  TCat* cats = reinterpret_cast<TCat*>(hp + z.cat);
  uint32_t* cw = reinterpret_cast<uint32_t*>(hp + z.bit);
  size_t blob = 0;
  int cat_at = 0, bit_at = 0;
  for (int i = 0; i < z.num_trees; ++i) {
    const Tree* tree = trees[i];
    const int nn = tree->num_leaves() - 1, nl = tree->num_leaves();
    LGAP_CHECK(nn <= 32767);  // (children are int16_t)
    const bool has_cat = HasCategoricalNode(tree);
    tt[i] = {static_cast<uint32_t>(blob), has_cat ? cat_at : 0, nn, nl};
    TNode* nodes = reinterpret_cast<TNode*>(hp + z.blob + blob);
    const auto& cb = tree->cat_boundaries_inner();
    for (int n = 0; n < nn; ++n) {
      const int8_t dt = tree->decision_type(n);
      const int thr = static_cast<int>(tree->threshold_in_bin(n));
      const bool cat = Tree::GetDecisionType(dt, kCategoricalMask);
      TCat unused;
      PackCompactNode(data->feature(tree->split_feature_inner(n)), dt, thr, tree->left_child(n), tree->right_child(n),
                      cat ? bit_at + cb[thr] : 0, cat ? cb[thr + 1] - cb[thr] : 0, &nodes[n],
                      has_cat ? &cats[cat_at + n] : &unused);
    }
    double* lv = reinterpret_cast<double*>(hp + z.blob + blob + sizeof(TNode) * nn);
    for (int l = 0; l < nl; ++l) lv[l] = tree->LeafOutput(l);
    if (nl & 1) lv[nl] = 0.0;  // (the blob's padding)
    if (has_cat) {
      const auto& ct = tree->cat_threshold_inner();
      for (size_t w = 0; w < ct.size(); ++w) cw[bit_at + w] = ct[w];
      cat_at += nn;
      bit_at += static_cast<int>(ct.size());
    }
    blob += ForestTreeBytes(nl);
  }
}

// the packed forest as LaunchTraverseForest takes it
struct ForestDev {
  const TForestTree* trees;
  const TForestRun* runs;
  const unsigned char* blob;
  const TCat* cats;
  const uint32_t* cat_bits;
  int num_trees, num_runs;
};
// base: the device copy of what PackCompactForest wrote
inline ForestDev CompactForestAt(const char* base, const ForestLayout& z) {
  return {reinterpret_cast<const TForestTree*>(base), reinterpret_cast<const TForestRun*>(base + z.run),
          reinterpret_cast<const unsigned char*>(base + z.blob), reinterpret_cast<const TCat*>(base + z.cat),
          reinterpret_cast<const uint32_t*>(base + z.bit), z.num_trees, static_cast<int>(z.runs.size())};
}

}  // namespace device
}  // namespace lgap
