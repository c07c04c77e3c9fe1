// Packed ensemble for prediction from raw feature rows (Booster.predict_device).
//
// The trees of [start_iteration, start_iteration + num_iteration) x num_tree_per_iteration are
// flattened into contiguous arrays in raw-feature space (real feature indices, fp64 thresholds,
// the raw-category bitsets), and the row walk and leaf output below are LGAP_HD: the HIP kernels
// (predict_kernels.hip) and the host loop (PredictPackedHost) execute the same source. They
// reproduce Tree::NumericalDecision, Tree::CategoricalDecision, Tree::GetLeaf, the one-leaf
// case and Tree::Predict (lgap/tree.h), on rows read the way PredictRows reads them.
// Free of HIP headers: plain C++ translation units include it.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "lgap/meta.h"

namespace lgap {

class GBDT;

namespace device {

// decision_type bits (lgap/tree.h): categorical, default-left, missing type << 2
constexpr int kPCategorical = 1;
constexpr int kPDefaultLeft = 2;
constexpr int kPMissingZero = 1;  // MissingType::Zero
constexpr int kPMissingNaN = 2;   // MissingType::NaN

// children >= 0 are nodes of the same tree, < 0 are ~leaf; int32, num_leaves is not bounded here
struct PNode {
  double threshold;  // categorical: index of the node's bitset in the tree's boundaries
  int32_t split_feature;
  int32_t left;
  int32_t right;
  uint8_t decision_type;
  uint8_t pad0, pad1, pad2;
};
static_assert(sizeof(PNode) == 24, "PNode is staged in LDS as 6 dwords");

struct PTree {
  int32_t node_off;  // first node in nodes[]
  int32_t leaf_off;  // first leaf in leaf_value[] / lin_const[] / lin_off[]
  int32_t num_leaves;
  int32_t cat_off;   // the tree's first entry in cat_boundaries[]
  int32_t is_linear;
};

// non-owning view (host or device pointers)
struct PackedView {
  const PNode* nodes = nullptr;
  const PTree* trees = nullptr;
  const int32_t* cat_boundaries = nullptr;  // per tree num_cat + 1 entries, offsets into cat_threshold
  const uint32_t* cat_threshold = nullptr;  // raw-category bitsets
  const double* leaf_value = nullptr;
  // linear trees: leaf (leaf_off + l) owns coefficients / features [lin_off[.], lin_off[. + 1])
  const double* lin_const = nullptr;
  const int32_t* lin_off = nullptr;
  const double* lin_coef = nullptr;
  const int32_t* lin_feat = nullptr;
  int num_trees = 0;
  int num_tree_per_iteration = 1;
  int num_iterations = 0;
  int average_output = 0;
};

struct PackedEnsemble {
  std::vector<PNode> nodes;
  std::vector<PTree> trees;
  std::vector<int32_t> cat_boundaries;
  std::vector<uint32_t> cat_threshold;
  std::vector<double> leaf_value;
  std::vector<double> lin_const;
  std::vector<int32_t> lin_off;
  std::vector<double> lin_coef;
  std::vector<int32_t> lin_feat;
  int num_tree_per_iteration = 1;
  int num_iterations = 0;
  bool average_output = false;

  PackedView View() const {
    PackedView v;
    v.nodes = nodes.data();
    v.trees = trees.data();
    v.cat_boundaries = cat_boundaries.data();
    v.cat_threshold = cat_threshold.data();
    v.leaf_value = leaf_value.data();
    v.lin_const = lin_const.data();
    v.lin_off = lin_off.data();
    v.lin_coef = lin_coef.data();
    v.lin_feat = lin_feat.data();
    v.num_trees = static_cast<int>(trees.size());
    v.num_tree_per_iteration = num_tree_per_iteration;
    v.num_iterations = num_iterations;
    v.average_output = average_output ? 1 : 0;
    return v;
  }
};

// Packs the iterations InitPredict selected (clamped like GBDT::InitPredict).
PackedEnsemble PackEnsemble(const GBDT& gbdt, int start_iteration, int num_iteration);

// what PredictRows computes per row
enum PredictMode : int { kPredictRaw = 0, kPredictLeaf = 1 };

// rows x PredictWidth(view, mode) doubles in out, by the shared walk in a host loop
void PredictPackedHost(const PackedView& view, const void* data, bool f64, int64_t nrow, int ncol, int mode,
                       double* out);
// the same result by the tree-parallel algorithm of k_predict_pairs / k_predict_fold in host
// loops: every (row, tree) pair into a [tree][row] array, then the shared fold
void PredictPackedHostTreeParallel(const PackedView& view, const void* data, bool f64, int64_t nrow, int ncol,
                                   int mode, double* out);

// memcpy, split over the OpenMP threads above a few MiB (the resident predictor's staging copies)
void CopyHostBytes(void* dst, const void* src, size_t bytes);

inline int PredictWidth(const PackedView& v, int mode) {
  return mode == kPredictLeaf ? v.num_trees : v.num_tree_per_iteration;
}

// ---- the shared walk --------------------------------------------------------------------

// Feature f of a dense row as the host predictor sees it: widened to fp64, a column the row
// does not have reads 0, and DenseSource::GetRow keeps only NaN and |v| > kZeroThreshold (the
// rest of the zero-filled row stays +0.0).
template <typename T>
LGAP_HD inline double PredFeature(const T* row, int ncol, int f) {
  if (f >= ncol) return 0.0;
  const double v = static_cast<double>(row[f]);
  return (__builtin_isnan(v) || fabs(v) > kZeroThreshold) ? v : 0.0;
}

// Tree::Decision: the next node (or ~leaf) from node `nd` for feature value fval; cat_b is the
// tree's slice of the boundaries.
LGAP_HD inline int PredDecide(const PNode& nd, double fval, const int32_t* cat_b, const uint32_t* cat_t) {
  // the fields by value: a choice between nd.left and nd.right stays a choice of registers
  const int dt = nd.decision_type;
  const int left = nd.left, right = nd.right;
  const double threshold = nd.threshold;
  if (dt & kPCategorical) {
    // NaN, negatives and values past the bitset go right. static_cast<int> of a value outside
    // int's range is what the host does with the x86 conversion (INT_MIN: right); the range
    // test says the same without depending on the conversion.
    if (__builtin_isnan(fval) || !(fval > -1.0 && fval < 2147483648.0)) return right;
    const int iv = static_cast<int>(fval);
    const int ci = static_cast<int>(threshold);
    const int b = cat_b[ci], e = cat_b[ci + 1];
    const int word = iv / 32;
    if (word >= e - b) return right;
    return ((cat_t[b + word] >> (iv % 32)) & 1u) ? left : right;
  }
  const int mt = (dt >> 2) & 3;
  if (__builtin_isnan(fval) && mt != kPMissingNaN) fval = 0.0;
  if ((mt == kPMissingZero && fval >= -kZeroThreshold && fval <= kZeroThreshold) ||
      (mt == kPMissingNaN && __builtin_isnan(fval))) {
    return (dt & kPDefaultLeft) ? left : right;
  }
  return fval <= threshold ? left : right;
}

// Tree::PredictLeafIndex over `nodes` (the tree's own nodes): 0 for a one-leaf tree
template <typename T>
LGAP_HD inline int PredLeaf(const PNode* nodes, int num_leaves, const int32_t* cat_b, const uint32_t* cat_t,
                            const T* row, int ncol) {
  if (num_leaves <= 1) return 0;
  int node = 0;
  while (node >= 0) {
    const PNode nd = nodes[node];
    node = PredDecide(nd, PredFeature(row, ncol, nd.split_feature), cat_b, cat_t);
  }
  return ~node;
}

// Tree::Predict's value at `leaf`; leaf_out is the leaf's plain output. A linear leaf adds
// const + sum(coeff * x) in feature order and returns the plain output at the first NaN. The
// products and sums stay separate operations (no FMA contraction): the host build has none.
template <typename T>
LGAP_HD inline double PredLeafOutput(const PackedView& v, const PTree& tr, int leaf, double leaf_out, const T* row,
                                     int ncol) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!tr.is_linear) return leaf_out;
  const int g = tr.leaf_off + leaf;
  double out = v.lin_const[g];
  for (int q = v.lin_off[g]; q < v.lin_off[g + 1]; ++q) {
    const double x = PredFeature(row, ncol, v.lin_feat[q]);
    if (__builtin_isnan(x)) return leaf_out;
    const double prod = v.lin_coef[q] * x;
    out = out + prod;
  }
  return out;
}

// ---- the tree-parallel form: one walk per (row, tree) pair, then a fold per (row, class) ----

// Tree `tree`'s value for one row: what the row-parallel walk adds to the row's accumulator
template <typename T>
LGAP_HD inline double PredPairValue(const PackedView& v, const PTree& tr, const PNode* nodes, const double* leaves,
                                    const T* row, int ncol) {
  const int leaf = PredLeaf(nodes, tr.num_leaves, v.cat_boundaries + tr.cat_off, v.cat_threshold, row, ncol);
  return PredLeafOutput(v, tr, leaf, leaves[leaf], row, ncol);
}

// Class k's raw score of row `row` from vals[tree][row] (rows `stride` apart): from 0.0, the
// trees k, k + K, ... added in ascending order, then average_output's division. The host's
// out[k] += Predict(x) order from the same starting value: the same bits.
LGAP_HD inline double PredFoldRow(const PackedView& v, const double* vals, int64_t stride, int64_t row, int k) {
  double acc = 0.0;
  for (int tree = k; tree < v.num_trees; tree += v.num_tree_per_iteration) {
    acc = acc + vals[static_cast<int64_t>(tree) * stride + row];
  }
  if (v.average_output && v.num_iterations > 0) acc /= v.num_iterations;
  return acc;
}

}  // namespace device
}  // namespace lgap
