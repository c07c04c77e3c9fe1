// Packer and host loop of the SHAP path pack (contrib_pack.h).
#include "device/contrib_pack.h"

#include <algorithm>

#include "lgap/boosting.h"
#include "lgap/log.h"
#include "lgap/tree.h"

namespace lgap {
namespace device {

ContribPack PackContrib(const GBDT& gbdt, int start_iteration, int num_iteration) {
  ContribPack cp;
  cp.pk = PackEnsemble(gbdt, start_iteration, num_iteration);
  cp.num_features = gbdt.MaxFeatureIdx() + 1;
  const int K = cp.pk.num_tree_per_iteration;
  const int total = gbdt.NumberOfTotalModel() / K;
  const int first = std::max(0, std::min(start_iteration, total)) * K;
  const int num_trees = static_cast<int>(cp.pk.trees.size());
  cp.ctrees.reserve(num_trees);
  std::vector<int> parent;                  // of a node; of leaf l at [L - 1 + l]
  std::vector<CEdge> up;                    // one leaf's edges, leaf to root
  std::vector<std::vector<CEdge>> per_elem;  // the same edges root to leaf, by element
  for (int i = 0; i < num_trees; ++i) {
    const Tree* t = gbdt.GetTree(first + i);
    if (t->is_linear()) {
      Log::Fatal("predict_contrib_device does not support linear trees (Booster.predict ignores their leaf "
                 "coefficients in SHAP values); use Booster.predict");
    }
    const int L = t->num_leaves();
    CTree ct;
    ct.expected_value = t->ExpectedValue();
    ct.path_off = static_cast<int32_t>(cp.paths.size());
    ct.num_paths = L > 1 ? L : 0;
    cp.ctrees.push_back(ct);
    if (L <= 1) continue;
    parent.assign(2 * static_cast<size_t>(L) - 1, -1);
    for (int n = 0; n < L - 1; ++n) {
      for (int c : {t->left_child(n), t->right_child(n)}) parent[c >= 0 ? c : L - 1 + ~c] = n;
    }
    for (int l = 0; l < L; ++l) {
      up.clear();
      for (int c = ~l, n = parent[L - 1 + l]; n >= 0; c = n, n = n > 0 ? parent[n] : -1) up.push_back(CEdge{n, c});
      if (up.empty() || up.back().node != 0) Log::Fatal("predict_contrib_device: leaf %d of a tree is not reachable", l);
      CPath path;
      path.leaf_value = t->LeafOutput(l);
      path.elem_off = static_cast<int32_t>(cp.elems.size());
      // root to leaf: group the edges by split feature, features in order of first appearance
      per_elem.clear();
      for (auto it = up.rbegin(); it != up.rend(); ++it) {
        const int f = t->split_feature(it->node);
        if (f < 0 || f >= cp.num_features) {
          Log::Fatal("predict_contrib_device: split feature %d outside the model's %d features", f, cp.num_features);
        }
        const double cnt_child = it->child >= 0 ? t->internal_count(it->child) : t->leaf_count(~it->child);
        const double frac = cnt_child / static_cast<double>(t->internal_count(it->node));
        size_t k = 0;
        while (k < per_elem.size() && cp.elems[path.elem_off + k].feature != f) ++k;
        if (k == per_elem.size()) {
          CElem e{};
          e.z = frac * 1.0;
          e.feature = f;
          cp.elems.push_back(e);
          per_elem.emplace_back();
        } else {
          CElem& e = cp.elems[path.elem_off + k];
          e.z = frac * e.z;
        }
        per_elem[k].push_back(*it);
      }
      path.num_elems = static_cast<int32_t>(per_elem.size());
      if (path.num_elems > kCMaxPathFeatures) {
        Log::Fatal("predict_contrib_device: a path splits on %d distinct features, the kernel holds %d "
                   "(kCMaxPathFeatures); use Booster.predict",
                   path.num_elems, kCMaxPathFeatures);
      }
      for (int k = 0; k < path.num_elems; ++k) {
        CElem& e = cp.elems[path.elem_off + k];
        e.edge_off = static_cast<int32_t>(cp.edges.size());
        e.num_edges = static_cast<int32_t>(per_elem[k].size());
        cp.edges.insert(cp.edges.end(), per_elem[k].begin(), per_elem[k].end());
      }
      if (cp.edges.size() > static_cast<size_t>(INT32_MAX)) {
        Log::Fatal("predict_contrib_device: the model slice has more than 2^31 path edges; use Booster.predict");
      }
      cp.max_path = std::max(cp.max_path, static_cast<int>(path.num_elems));
      cp.paths.push_back(path);
    }
  }
  return cp;
}

namespace {

template <typename T>
void HostLoop(const ContribPack& pack, const T* data, int64_t nrow, int ncol, double* out) {
  const ContribView v = pack.View();
  const int width = ContribWidth(v);
#pragma omp parallel
  {
    std::vector<double> w(static_cast<size_t>(pack.max_path) + 1);
#pragma omp for schedule(static)
    for (int64_t i = 0; i < nrow; ++i) {
      double* o = out + i * width;
      std::fill(o, o + width, 0.0);
      ContribRow(v, data + i * ncol, ncol, w.data(), 1, o, 1);
    }
  }
}

}  // namespace

void ContribPackedHost(const ContribPack& pack, const void* data, bool f64, int64_t nrow, int ncol, double* out) {
  if (f64) HostLoop(pack, static_cast<const double*>(data), nrow, ncol, out);
  else HostLoop(pack, static_cast<const float*>(data), nrow, ncol, out);
}

}  // namespace device
}  // namespace lgap
