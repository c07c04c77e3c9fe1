// Packer and host loop of the packed prediction ensemble (predict_pack.h).
#include "device/predict_pack.h"

#include <algorithm>
#include <cstring>

#include "lgap/boosting.h"
#include "lgap/log.h"
#include "lgap/tree.h"

namespace lgap {
namespace device {

PackedEnsemble PackEnsemble(const GBDT& gbdt, int start_iteration, int num_iteration) {
  PackedEnsemble pk;
  const int K = std::max(1, gbdt.NumModelPerIteration());
  const int total = gbdt.NumberOfTotalModel() / K;
  start_iteration = std::max(0, std::min(start_iteration, total));
  int iters = total - start_iteration;
  if (num_iteration > 0) iters = std::min(num_iteration, iters);
  pk.num_tree_per_iteration = K;
  pk.num_iterations = iters;
  pk.average_output = gbdt.average_output();
  const int num_trees = iters * K;
  pk.trees.reserve(num_trees);
  pk.lin_off.push_back(0);
  for (int i = 0; i < num_trees; ++i) {
    const Tree* t = gbdt.GetTree(start_iteration * K + i);
    const int L = t->num_leaves();
    if (pk.nodes.size() + static_cast<size_t>(L) > static_cast<size_t>(INT32_MAX)) {
      Log::Fatal("predict_device: the model slice has more than 2^31 nodes");
    }
    PTree pt;
    pt.node_off = static_cast<int32_t>(pk.nodes.size());
    pt.leaf_off = static_cast<int32_t>(pk.leaf_value.size());
    pt.num_leaves = L;
    pt.cat_off = static_cast<int32_t>(pk.cat_boundaries.size());
    pt.is_linear = t->is_linear() ? 1 : 0;
    for (int n = 0; n < L - 1; ++n) {
      PNode nd;
      nd.threshold = t->threshold(n);
      nd.split_feature = t->split_feature(n);
      nd.left = t->left_child(n);
      nd.right = t->right_child(n);
      nd.decision_type = static_cast<uint8_t>(t->decision_type(n));
      nd.pad0 = nd.pad1 = nd.pad2 = 0;
      pk.nodes.push_back(nd);
    }
    if (t->num_cat() > 0) {
      // the tree's boundaries, rebased onto the ensemble's bitset words
      const int32_t base = static_cast<int32_t>(pk.cat_threshold.size());
      for (int b : t->cat_boundaries()) pk.cat_boundaries.push_back(base + b);
      pk.cat_threshold.insert(pk.cat_threshold.end(), t->cat_threshold().begin(), t->cat_threshold().end());
    }
    for (int l = 0; l < L; ++l) {
      pk.leaf_value.push_back(t->LeafOutput(l));
      if (t->is_linear()) {
        pk.lin_const.push_back(t->LeafConst(l));
        const auto& coef = t->LeafCoeffs(l);
        const auto& feat = t->LeafFeatures(l);
        // Tree::Predict runs over the feature list
        for (size_t q = 0; q < feat.size(); ++q) {
          pk.lin_coef.push_back(coef[q]);
          pk.lin_feat.push_back(feat[q]);
        }
      } else {
        pk.lin_const.push_back(0.0);
      }
      pk.lin_off.push_back(static_cast<int32_t>(pk.lin_coef.size()));
    }
    pk.trees.push_back(pt);
  }
  return pk;
}

namespace {

template <typename T>
void HostLoop(const PackedView& v, const T* data, int64_t nrow, int ncol, int mode, double* out) {
  const int K = v.num_tree_per_iteration;
  const int width = PredictWidth(v, mode);
#pragma omp parallel for schedule(static)
  for (int64_t i = 0; i < nrow; ++i) {
    const T* row = data + i * ncol;
    double* o = out + i * width;
    if (mode != kPredictLeaf) std::fill(o, o + K, 0.0);
    for (int t = 0; t < v.num_trees; ++t) {
      const PTree tr = v.trees[t];
      const int leaf = PredLeaf(v.nodes + tr.node_off, tr.num_leaves, v.cat_boundaries + tr.cat_off, v.cat_threshold,
                                row, ncol);
      if (mode == kPredictLeaf) {
        o[t] = leaf;
      } else {
        o[t % K] += PredLeafOutput(v, tr, leaf, v.leaf_value[tr.leaf_off + leaf], row, ncol);
      }
    }
    if (mode != kPredictLeaf && v.average_output && v.num_iterations > 0) {
      for (int k = 0; k < K; ++k) o[k] /= v.num_iterations;
    }
  }
}

template <typename T>
void HostPairsFold(const PackedView& v, const T* data, int64_t nrow, int ncol, int mode, double* out) {
  const int K = v.num_tree_per_iteration;
  const int64_t pairs = nrow * v.num_trees;
  if (mode == kPredictLeaf) {
#pragma omp parallel for schedule(static)
    for (int64_t p = 0; p < pairs; ++p) {
      const int64_t t = p / nrow, i = p % nrow;
      const PTree tr = v.trees[t];
      out[i * v.num_trees + t] = PredLeaf(v.nodes + tr.node_off, tr.num_leaves, v.cat_boundaries + tr.cat_off,
                                          v.cat_threshold, data + i * ncol, ncol);
    }
    return;
  }
  std::vector<double> vals(static_cast<size_t>(pairs));
#pragma omp parallel for schedule(static)
  for (int64_t p = 0; p < pairs; ++p) {
    const int64_t t = p / nrow, i = p % nrow;
    const PTree tr = v.trees[t];
    vals[p] = PredPairValue(v, tr, v.nodes + tr.node_off, v.leaf_value + tr.leaf_off, data + i * ncol, ncol);
  }
#pragma omp parallel for schedule(static)
  for (int64_t q = 0; q < nrow * K; ++q) {
    const int64_t k = q / nrow, i = q % nrow;
    out[i * K + k] = PredFoldRow(v, vals.data(), nrow, i, static_cast<int>(k));
  }
}

}  // namespace

void PredictPackedHostTreeParallel(const PackedView& view, const void* data, bool f64, int64_t nrow, int ncol,
                                   int mode, double* out) {
  if (nrow <= 0) return;
  if (f64) HostPairsFold(view, static_cast<const double*>(data), nrow, ncol, mode, out);
  else HostPairsFold(view, static_cast<const float*>(data), nrow, ncol, mode, out);
}

void CopyHostBytes(void* dst, const void* src, size_t bytes) {
  constexpr size_t kBlock = size_t(1) << 20;
  if (bytes <= 4 * kBlock) {
    std::memcpy(dst, src, bytes);
    return;
  }
  const int64_t blocks = static_cast<int64_t>((bytes + kBlock - 1) / kBlock);
#pragma omp parallel for schedule(static)
  for (int64_t b = 0; b < blocks; ++b) {
    const size_t off = static_cast<size_t>(b) * kBlock;
    std::memcpy(static_cast<char*>(dst) + off, static_cast<const char*>(src) + off, std::min(kBlock, bytes - off));
  }
}

void PredictPackedHost(const PackedView& view, const void* data, bool f64, int64_t nrow, int ncol, int mode,
                       double* out) {
  if (f64) HostLoop(view, static_cast<const double*>(data), nrow, ncol, mode, out);
  else HostLoop(view, static_cast<const float*>(data), nrow, ncol, mode, out);
}

}  // namespace device
}  // namespace lgap
