// Metric evaluation where the score lives: every metric family of the device learner over one
// view of a device-resident score (the training set's or a device validation set's). Only the
// metric's sums come back (no score download). The kernels are grad_kernels.h (pointwise,
// multiclass) and metric_kernels.h (AUC, auc_mu, query metrics).
#pragma once

#include <map>
#include <memory>
#include <vector>

#include "device/hip_common.h"
#include "lgap/pointwise_metric.h"
#include "lgap/rank_metric_spec.h"

namespace lgap {
namespace device {

// a class-major device score of `len` doubles over n rows with the rows' labels / weights
struct ScoreView {
  const double* score = nullptr;
  size_t len = 0;
  const float* label = nullptr;   // device; nullptr: the set has no labels (no metric applies)
  const float* weight = nullptr;  // device; nullptr: 1
  const void* host_label = nullptr;  // the dataset's labels (identity check of metric specs)
  int n = 0;
};

// Every entry point returns false, with nothing launched, for a view or spec it does not hold
// (the caller evaluates on the host); otherwise it returns after the sums have arrived.
class MetricEval {
 public:
  // sum of the pointwise metric's weighted row loss over class k; `timer`: the phase name
  bool Pointwise(const ScoreView& v, const PwMetricParams& p, int k, const char* timer, double* sum, hipStream_t s);
  // the multiclass metric's weighted loss sum
  bool Multi(const ScoreView& v, const MultiMetricParams& p, double* sum, hipStream_t s);
  // auc_mu per-pair accumulators S_ij (pairs i < j in row-major order)
  bool AucMu(const ScoreView& v, const AucMuSpec& spec, std::vector<double>* out, hipStream_t s);
  // ranking / AUC metric of class k: raw sums for Metric::FinishRank. The metric's per-query
  // tables are uploaded once per metric.
  bool Rank(const ScoreView& v, const RankMetricSpec& spec, int k, std::vector<double>* out, hipStream_t s);

 private:
  static constexpr int kMetricBlocks = 1024;
  // the view holds class k of n > 0 labelled rows
  static bool Holds(const ScoreView& v, int k) {
    return v.label != nullptr && v.n > 0 && v.len >= static_cast<size_t>(k + 1) * v.n;
  }
  double ReadSum(hipStream_t s);

  // per-metric device tables of the ranking / AUC metrics, keyed by the metric
  struct RankEvalState {
    int kind = -1, n = 0, nq = 0;
    const void* host_label = nullptr;
    const void* host_qb = nullptr;
    std::vector<int> ks;
    DevBuf<int> qb, npos, ks_dev;
    DevBuf<float> qw;
    DevBuf<double> inv_max, gain, disc, out;
    DevBuf<char> scratch;
  };
  std::map<const void*, std::unique_ptr<RankEvalState>> rank_states_;
  // auc_mu tables per metric: the class-ordered row index, one pair's scored rows, the pairs' sums
  struct AucMuState {
    int n = 0;
    const void* host_label = nullptr;
    DevBuf<int> idx;
    DevBuf<double> dist, out;
    DevBuf<float> lab, w;
    DevBuf<char> scratch;
  };
  std::map<const void*, std::unique_ptr<AucMuState>> aucmu_states_;
  DevBuf<double> partial_;  // kMetricBlocks block sums, then the total
  PinnedBuf<double> pin_;
};

}  // namespace device
}  // namespace lgap
