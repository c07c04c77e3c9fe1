// Path pack and per-row function of SHAP values on the device (Booster.predict_contrib_device).
//
// Next to the packed ensemble of predict_pack.h (nodes, bitsets: the decisions), every leaf of
// every selected tree gets its root-to-leaf path as unique features (the GPUTreeShap path form):
// one element per distinct split feature on the path, holding the feature, z (the product of the
// child / parent data-count fractions of that feature's edges, multiplied in path order) and
// the edges themselves as (node, child taken). A row's "one fraction" o of an element is 1 when
// PredDecide takes every one of its edges and 0 otherwise, so repeated features need no Unwind.
// ContribRow below is LGAP_HD: the HIP kernel (contrib_kernels.hip) and the host loop
// (ContribPackedHost) execute the same source, with Tree::TreeSHAP's Extend / UnwoundSum
// arithmetic (model/tree.cpp). The host recursion associates the same sums in another order, so
// the two agree to rounding, not bit for bit; the expected-value column is bit-identical.
// Free of HIP headers: plain C++ translation units include it.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "device/predict_pack.h"

namespace lgap {
namespace device {

// Unique split features on one root-to-leaf path that the kernel holds: the row's one
// fractions of a path are the bits of one 64-bit word. Longer paths are refused at pack time.
constexpr int kCMaxPathFeatures = 64;

struct CEdge {
  int32_t node;   // node of the tree (tree-local index)
  int32_t child;  // the child the path takes, as PNode::left / right hold it
};

struct CElem {
  double z;
  int32_t feature;
  int32_t edge_off;  // first edge in edges[]
  int32_t num_edges;
  int32_t pad;
};
static_assert(sizeof(CElem) == 24, "CElem is read as 6 dwords");

struct CPath {
  double leaf_value;
  int32_t elem_off;  // first element in elems[]
  int32_t num_elems;
};

struct CTree {
  double expected_value;  // Tree::ExpectedValue()
  int32_t path_off;       // first path in paths[]; leaf order
  int32_t num_paths;      // 0 for a one-leaf tree
};

// non-owning view (host or device pointers)
struct ContribView {
  PackedView pv;  // nodes, trees and bitsets of the same selected trees
  const CTree* ctrees = nullptr;
  const CPath* paths = nullptr;
  const CElem* elems = nullptr;
  const CEdge* edges = nullptr;
  int num_features = 0;  // max_feature_idx + 1: a class block is num_features + 1 columns
};

struct ContribPack {
  PackedEnsemble pk;
  std::vector<CTree> ctrees;
  std::vector<CPath> paths;
  std::vector<CElem> elems;
  std::vector<CEdge> edges;
  int num_features = 0;
  int max_path = 0;  // most unique features on any path

  ContribView View() const {
    ContribView v;
    v.pv = pk.View();
    v.ctrees = ctrees.data();
    v.paths = paths.data();
    v.elems = elems.data();
    v.edges = edges.data();
    v.num_features = num_features;
    return v;
  }
};

// Packs the iterations InitPredict selected. Fatal for linear trees and for a path with more than
// kCMaxPathFeatures unique features.
ContribPack PackContrib(const GBDT& gbdt, int start_iteration, int num_iteration);

inline int ContribWidth(const ContribView& v) { return v.pv.num_tree_per_iteration * (v.num_features + 1); }

// rows x ContribWidth doubles in out, by ContribRow in a host loop
void ContribPackedHost(const ContribPack& pack, const void* data, bool f64, int64_t nrow, int ncol, double* out);

// ---- the shared per-row function --------------------------------------------------------

// SHAP values of one row over all trees in order, paths in leaf order. w is the row's weight
// array, max_path + 1 doubles at stride ws; phi the row's ContribWidth values at stride ps,
// zeroed by the caller. Per path: the one fractions, Extend's recurrence over the root element
// and the path's elements, then per element UnwoundSum and phi += w * (o - z) * leaf value.
// Products, sums and quotients stay separate operations (no FMA contraction), as on the host.
template <typename T>
LGAP_HD inline void ContribRow(const ContribView& v, const T* row, int ncol, double* w, size_t ws, double* phi,
                               size_t ps) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int K = v.pv.num_tree_per_iteration;
  const int block = v.num_features + 1;
  for (int t = 0; t < v.pv.num_trees; ++t) {
    const PTree tr = v.pv.trees[t];
    const CTree ct = v.ctrees[t];
    double* out = phi + static_cast<size_t>(t % K) * block * ps;
    out[static_cast<size_t>(v.num_features) * ps] = out[static_cast<size_t>(v.num_features) * ps] + ct.expected_value;
    const PNode* nodes = v.pv.nodes + tr.node_off;
    const int32_t* cat_b = v.pv.cat_boundaries + tr.cat_off;
    for (int p = 0; p < ct.num_paths; ++p) {
      const CPath path = v.paths[ct.path_off + p];
      const CElem* el = v.elems + path.elem_off;
      const int m = path.num_elems;
      // Extend: the root element (z = 1, o = 1) at depth 0, element j at depth j + 1
      uint64_t ones = 0;
      w[0] = 1.0;
      for (int j = 0; j < m; ++j) {
        const CElem e = el[j];
        const double fval = PredFeature(row, ncol, e.feature);
        bool hot = true;
        for (int q = 0; q < e.num_edges; ++q) {
          const CEdge ed = v.edges[e.edge_off + q];
          hot = hot && PredDecide(nodes[ed.node], fval, cat_b, v.pv.cat_threshold) == ed.child;
        }
        if (hot) ones |= uint64_t(1) << j;
        const double o = hot ? 1.0 : 0.0;
        const int d = j + 1;
        const double dp1 = static_cast<double>(d + 1);
        w[d * ws] = 0.0;
        for (int i = d - 1; i >= 0; --i) {
          const double wi = w[i * ws];
          const double up = o * wi;
          const double up2 = up * (i + 1);
          const double up3 = up2 / dp1;
          w[(i + 1) * ws] = w[(i + 1) * ws] + up3;
          const double dn = e.z * wi;
          const double dn2 = dn * (d - i);
          w[i * ws] = dn2 / dp1;
        }
      }
      const int d = m;
      const double dp1 = static_cast<double>(d + 1);
      const double wd = w[d * ws];
      for (int j = 0; j < m; ++j) {
        const CElem e = el[j];
        const bool hot = (ones >> j) & 1u;
        const double o = hot ? 1.0 : 0.0;
        // UnwoundSum of element j
        double next = wd, total = 0.0;
        for (int i = d - 1; i >= 0; --i) {
          const double wi = w[i * ws];
          if (hot) {
            const double a = next * dp1;
            const double b = static_cast<double>(i + 1) * o;
            const double tt = a / b;
            total = total + tt;
            const double c = (d - i) / dp1;
            const double s = tt * e.z;
            const double s2 = s * c;
            next = wi - s2;
          } else {
            const double a = wi / e.z;
            const double c = (d - i) / dp1;
            const double tt = a / c;
            total = total + tt;
          }
        }
        const double scale = total * (o - e.z);
        const double add = scale * path.leaf_value;
        double* dst = out + static_cast<size_t>(e.feature) * ps;
        *dst = *dst + add;
      }
    }
  }
}

}  // namespace device
}  // namespace lgap
