// Metric evaluation over a device score view (see metric_eval.h). Host code only: the kernels
// are in grad_kernels.hip and metric_kernels.hip.
#include "device/metric_eval.h"

#include <algorithm>
#include <cmath>

#include "device/grad_kernels.h"
#include "device/metric_kernels.h"
#include "lgap/common.h"

namespace lgap {
namespace device {

// the total the pointwise / multiclass launch left behind its block sums
double MetricEval::ReadSum(hipStream_t s) {
  double* h = pin_.Get(RankMetricSpec::kMaxEvalAt);
  HIP_CHECK(hipMemcpyAsync(h, partial_.get() + kMetricBlocks, sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  return h[0];
}

bool MetricEval::Pointwise(const ScoreView& v, const PwMetricParams& p, int k, const char* timer, double* sum,
                           hipStream_t s) {
  if (!Holds(v, k)) return false;
  ScopedTimer scoped(timer);
  if (partial_.size() < static_cast<size_t>(kMetricBlocks + 1)) partial_.Resize(kMetricBlocks + 1);
  LaunchPointwiseMetric(p, v.score + static_cast<size_t>(k) * v.n, v.label, v.weight, v.n, partial_.get(), kMetricBlocks,
                        partial_.get() + kMetricBlocks, s);
  *sum = ReadSum(s);
  return true;
}

bool MetricEval::Multi(const ScoreView& v, const MultiMetricParams& p, double* sum, hipStream_t s) {
  if (!Holds(v, p.num_class - 1)) return false;
  ScopedTimer timer("Device::EvalMultiMetric");
  if (partial_.size() < static_cast<size_t>(kMetricBlocks + 1)) partial_.Resize(kMetricBlocks + 1);
  LaunchMultiMetric(p, v.score, v.label, v.weight, v.n, partial_.get(), kMetricBlocks, partial_.get() + kMetricBlocks, s);
  *sum = ReadSum(s);
  return true;
}

bool MetricEval::AucMu(const ScoreView& v, const AucMuSpec& spec, std::vector<double>* out, hipStream_t s) {
  const int K = spec.num_class;
  if (K < 2 || K > kAucMuMaxClass || spec.sorted == nullptr || spec.sizes == nullptr || spec.cw == nullptr) return false;
  if (!Holds(v, K - 1)) return false;
  const int n = v.n;
  if (spec.num_data != n || spec.label != v.host_label || (spec.weights != nullptr) != (v.weight != nullptr)) return false;
  if (static_cast<int>(spec.sorted->size()) != n || static_cast<int>(spec.sizes->size()) != K) return false;
  ScopedTimer timer("Device::EvalAucMu");
  auto& slot = aucmu_states_[spec.owner];
  const int npairs = K * (K - 1) / 2;
  int maxpair = 0;
  for (int i = 0; i < K; ++i)
    for (int j = i + 1; j < K; ++j) maxpair = std::max(maxpair, (*spec.sizes)[i] + (*spec.sizes)[j]);
  if (!slot || slot->n != n || slot->host_label != v.host_label) {
    slot = std::make_unique<AucMuState>();
    slot->n = n;
    slot->host_label = v.host_label;
    std::vector<int> idx(spec.sorted->begin(), spec.sorted->end());
    slot->idx.Upload(idx, s);
    HIP_CHECK(hipStreamSynchronize(s));  // (idx is a local staging vector)
    slot->dist.Resize(std::max(maxpair, 1));
    slot->lab.Resize(std::max(maxpair, 1));
    slot->w.Resize(std::max(maxpair, 1));
    slot->scratch.Resize(AucScratchBytes(std::max(maxpair, 1)));
    slot->out.Resize(kAucOutWords * static_cast<size_t>(npairs));
  }
  AucMuState& st = *slot;
  AucMuPairArgs pa;
  pa.score = v.score;
  pa.n = n;
  pa.K = K;
  pa.idx = st.idx.get();
  pa.weight = v.weight;
  pa.out_score = st.dist.get();
  pa.out_label = st.lab.get();
  pa.out_w = st.w.get();
  const auto& cw = *spec.cw;
  int istart = 0, q = 0;
  for (int i = 0; i < K; ++i) {
    int jstart = istart + (*spec.sizes)[i];
    for (int j = i + 1; j < K; ++j, ++q) {
      for (int c = 0; c < K; ++c) pa.v[c] = cw[i][c] - cw[j][c];
      pa.t1 = pa.v[i] - pa.v[j];
      pa.istart = istart;
      pa.ni = (*spec.sizes)[i];
      pa.jstart = jstart;
      pa.nj = (*spec.sizes)[j];
      LaunchAucMuPair(pa, s);
      LaunchAucMetric(false, st.dist.get(), st.lab.get(), v.weight != nullptr ? st.w.get() : nullptr, pa.ni + pa.nj,
                      st.scratch.get(), st.scratch.size(), st.out.get() + kAucOutWords * q, s);
      jstart += (*spec.sizes)[j];
    }
    istart += (*spec.sizes)[i];
  }
  std::vector<double> h(kAucOutWords * static_cast<size_t>(npairs));
  st.out.Download(h.data(), h.size(), s);
  HIP_CHECK(hipStreamSynchronize(s));
  out->assign(npairs, 0.0);
  for (int p = 0; p < npairs; ++p) (*out)[p] = h[kAucOutWords * p];
  return true;
}

bool MetricEval::Rank(const ScoreView& v, const RankMetricSpec& spec, int k, std::vector<double>* out, hipStream_t s) {
  if (!Holds(v, k)) return false;
  const int n = v.n;
  const double* score = v.score + static_cast<size_t>(k) * n;
  if (spec.num_data != n || spec.label != v.host_label) return false;
  if ((spec.weights != nullptr) != (v.weight != nullptr)) return false;
  const bool query = spec.kind >= RankMetricSpec::kNDCG;
  if (query && (spec.num_queries <= 0 || spec.query_boundaries == nullptr || spec.eval_at.empty() ||
                spec.eval_at.size() > static_cast<size_t>(RankMetricSpec::kMaxEvalAt))) {
    return false;
  }
  ScopedTimer timer("Device::EvalRankMetric");
  auto& slot = rank_states_[spec.owner];
  if (!slot || slot->kind != spec.kind || slot->n != n || slot->nq != spec.num_queries || slot->host_label != v.host_label ||
      slot->host_qb != static_cast<const void*>(spec.query_boundaries) || slot->ks != spec.eval_at) {
    // built aside and installed only when complete: a rejected spec leaves no half-built
    // state behind a matching key
    auto fresh = std::make_unique<RankEvalState>();
    RankEvalState& r = *fresh;
    r.kind = spec.kind;
    r.n = n;
    r.nq = spec.num_queries;
    r.host_label = v.host_label;
    r.host_qb = spec.query_boundaries;
    r.ks = spec.eval_at;
    if (query) {
      const int nq = spec.num_queries, ne = static_cast<int>(spec.eval_at.size());
      std::vector<int> qb(spec.query_boundaries, spec.query_boundaries + nq + 1);
      int maxq = 1;
      for (int q = 0; q < nq; ++q) maxq = std::max(maxq, qb[q + 1] - qb[q]);
      r.qb.Upload(qb, s);
      if (spec.query_weights) r.qw.Upload(spec.query_weights, nq, s);
      r.ks_dev.Upload(spec.eval_at, s);
      if (spec.kind == RankMetricSpec::kNDCG) {
        if (spec.inv_max.size() != static_cast<size_t>(nq) * ne || spec.label_gain.empty()) return false;
        r.inv_max.Upload(spec.inv_max, s);
        r.gain.Upload(spec.label_gain, s);
        std::vector<double> disc(maxq);  // DCGCalculator::Init's discount table
        for (int i = 0; i < maxq; ++i) disc[i] = 1.0 / std::log2(2.0 + i);
        r.disc.Upload(disc, s);
      } else if (spec.kind == RankMetricSpec::kMAP) {
        if (spec.npos.size() != static_cast<size_t>(nq)) return false;
        r.npos.Upload(spec.npos, s);
      }
      r.scratch.Resize(QueryMetricScratchBytes(n, nq, ne));
    } else {
      r.scratch.Resize(AucScratchBytes(n));
    }
    r.out.Resize(RankMetricSpec::kMaxEvalAt);
    // the uploads' host sources (qb, disc, ...) are locals of this scope
    HIP_CHECK(hipStreamSynchronize(s));
    slot = std::move(fresh);
  }
  RankEvalState& r = *slot;
  int nout = kAucOutWords;
  if (query) {
    QueryMetricArgs qa;
    qa.kind = spec.kind;
    qa.qb = r.qb.get();
    qa.nq = r.nq;
    qa.qw = r.qw.size() ? r.qw.get() : nullptr;
    qa.inv_max = r.inv_max.size() ? r.inv_max.get() : nullptr;
    qa.npos = r.npos.size() ? r.npos.get() : nullptr;
    qa.ks = r.ks_dev.get();
    qa.ne = static_cast<int>(r.ks.size());
    qa.gain = r.gain.size() ? r.gain.get() : nullptr;
    qa.ngain = static_cast<int>(r.gain.size());
    qa.disc = r.disc.size() ? r.disc.get() : nullptr;
    LaunchQueryMetric(qa, score, v.label, n, r.scratch.get(), r.scratch.size(), r.out.get(), s);
    nout = qa.ne;
  } else {
    LaunchAucMetric(spec.kind == RankMetricSpec::kAveragePrecision, score, v.label, v.weight, n, r.scratch.get(),
                    r.scratch.size(), r.out.get(), s);
  }
  double* h = pin_.Get(RankMetricSpec::kMaxEvalAt);
  HIP_CHECK(hipMemcpyAsync(h, r.out.get(), sizeof(double) * nout, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  out->assign(h, h + nout);
  return true;
}

}  // namespace device
}  // namespace lgap
