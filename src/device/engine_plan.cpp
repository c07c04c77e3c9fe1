#include "device/engine_plan.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "device/frontier_shape.h"
#include "learner/leaf_constraints.h"
#include "lgap/log.h"

namespace lgap {
namespace device {

DataShape ShapeOf(const Dataset* train) {
  DataShape s;
  if (train == nullptr) return s;
  s.has_data = true;
  s.total_bins = train->num_total_bin();
  s.features = train->num_features();
  s.has_raw = train->has_raw();
  for (int f = 0; f < train->num_features(); ++f) {
    const FeatureInfo& fi = train->feature(f);
    s.max_bin = std::max(s.max_bin, fi.num_bin);
    if (fi.bin_type != BinType::Categorical) continue;
    s.has_categorical = true;
    s.max_cat_bin = std::max(s.max_cat_bin, fi.num_bin);
  }
  return s;
}

RoutingEnv ReadRoutingEnv() {
  RoutingEnv r;
  auto is_off = [](const char* name) {
    const char* e = std::getenv(name);
    return e != nullptr && e[0] == '0';
  };
  r.frontier_off = is_off("LGAP_FRONTIER");
  r.frontier_dp_off = is_off("LGAP_FRONTIER_DP");
  if (const char* e = std::getenv("LGAP_DP_TRANSPORT")) {
    const std::string& t = r.dp_transport_text = e;
    r.dp_transport = t == "auto" ? DpTransport::kAuto : t == "xgmi" ? DpTransport::kXgmi
                     : t == "collective" ? DpTransport::kCollective
                     : t == "allreduce"  ? DpTransport::kAllreduce : DpTransport::kOther;
  }
  if (const char* e = std::getenv("LGAP_DEVICE_DP_TRANSPORT")) r.device_dp_host = std::strcmp(e, "host") == 0;
  if (const char* e = std::getenv("LGAP_DEVICE_HIST_BUDGET_MB")) {
    r.hist_budget_set = true;
    r.hist_budget_mb = std::atof(e);
  }
  if (const char* e = std::getenv("LGAP_FORCE_DEVICE_DP")) {
    r.force_dp = std::strcmp(e, "voting") == 0 ? ForceDP::kVoting : e[0] == '1' ? ForceDP::kData : ForceDP::kOff;
  }
  return r;
}

const char* EngineName(Engine e) {
  return e == Engine::kHostPolicy ? "host split policy" : e == Engine::kFrontier ? "frontier engine" : "sequential chain";
}

EnginePlan PlanEngine(const PlanInputs& in) {
  const Config* c = in.config;
  const DataShape& d = in.shape;
  const RoutingEnv& env = in.env;
  const std::string& type = in.learner_type;
  EnginePlan p;

  // ---- the device learner's parallel mode
  if (type != "serial" && type != "data" && type != "feature" && type != "voting") {
    Log::Fatal("Unknown tree learner type %s", type.c_str());
  }
  p.mode = type == "data" ? ParallelMode::kData : type == "feature" ? ParallelMode::kFeature
           : type == "voting" ? ParallelMode::kVoting : ParallelMode::kSerial;
  const bool forced_dp = in.comm_exists && env.force_dp != ForceDP::kOff;
  if (forced_dp && p.mode == ParallelMode::kSerial) {
    p.mode = env.force_dp == ForceDP::kVoting ? ParallelMode::kVoting : ParallelMode::kData;
  }
  const bool multi = in.comm_active || in.host_staged || forced_dp;
  // voting: a one-rank communicator also runs the voting path (single-GPU rehearsal)
  p.voting = p.mode == ParallelMode::kVoting && (multi || in.comm_exists);
  p.owner_scan = (p.mode == ParallelMode::kData || p.mode == ParallelMode::kFeature) && multi;
  p.distributed = (p.owner_scan && p.mode == ParallelMode::kData) || p.voting;

  // ---- what the configuration asks of the frontier's select
  const bool extra = c->extra_trees, bynode = c->feature_fraction_bynode < 1.0;
  const bool forced_splits = !c->forcedsplits_filename.empty();
  const size_t sets = c->interaction_constraints_vector.size();
  const bool mono = !c->monotone_constraints.empty() && c->monotone_constraints_method != "basic";
  p.cegb_coupled = !c->cegb_penalty_feature_coupled.empty();
  p.cegb_lazy = !c->cegb_penalty_feature_lazy.empty();
  const bool feature_pens = p.cegb_coupled || p.cegb_lazy;
  p.raw_cands = feature_pens || bynode;
  p.mono_inter = mono && c->monotone_constraints_method == "intermediate";
  p.bynode_on_device = bynode && sets > 0;

  // the frontier's fixed resources: constraint words, node capacity, the scan's LDS, the select's LDS
  // image of the nodes (+ F bytes each of raw-candidate flags and by-node scratch, + the monotone image)
  auto shape_fits = [&](bool raw, bool mono_inter) {
    if (sets > 64 * static_cast<size_t>(kFrontierIcWords)) return false;
    if (!d.has_data) return c->num_leaves <= 256;  // (no data yet: a conservative shape)
    if (env.frontier_off) return false;
    const int L = std::max(2, c->num_leaves), F = d.features, C = FrontierCapacityFor(L, d.total_bins);
    if (C > kFrontierMaxNodes || F <= 0 || FrontierScanLds(d.max_bin, d.max_cat_bin) > kFrontierLdsLimit) return false;
    return FrontierSelectLds(C, L) + (raw ? 2 * (F + 16) : 0) + (mono_inter ? FrontierSelectMonoLds(C, L, F) : 0) <=
           kFrontierLdsLimit;
  };

  // ---- the device learner's engine: the frontier on one device, or data / voting / feature parallel
  // over a communicator or the host-staged rehearsal transport; else the sequential chain
  const bool serial = p.mode == ParallelMode::kSerial;
  const bool link = in.comm_exists || in.host_staged;
  const bool fdata = p.mode == ParallelMode::kData && p.owner_scan && link && !env.frontier_dp_off;
  const bool fvoting = p.voting && link;
  const bool ffeature = p.mode == ParallelMode::kFeature && p.owner_scan && link;
  bool frontier = serial || fdata || fvoting || ffeature;
  // extra trees: one device, or voting on numerical data (the global pass's redraws are identical
  // on every rank only when no draw depends on local data: categorical draws count the local
  // histogram's used bins). By-node masks follow the host's draw order: one device.
  if (extra && !serial && !(fvoting && !d.has_categorical)) frontier = false;
  if (bynode && !serial) frontier = false;
  // (forced splits by the file name: whether it parses to any split is known after the engine is)
  if (p.mono_inter && (!serial || p.raw_cands || extra || forced_splits)) frontier = false;
  // KNOWN: voting with cegb_penalty_split, or with numerical extra_trees,
  // on a shape the frontier cannot hold lands on the sequential chain, whose vote scan neither
  // subtracts the penalty nor redraws thresholds. Kept as it was routed; the fix is a host reason.
  if (frontier && !shape_fits(p.raw_cands, p.mono_inter)) frontier = false;
  // raw per-feature candidates, forced splits and extra trees need every feature's scan on every
  // rank: they keep the all-reduce, as does LGAP_DP_TRANSPORT=allreduce (A/B)
  const bool owner = !p.raw_cands && !forced_splits && !extra && env.dp_transport != DpTransport::kAllreduce;
  if (frontier) {
    p.frontier = serial ? FrontierMode::kSerial : fvoting ? FrontierMode::kVoting : ffeature ? FrontierMode::kFeature
                 : owner ? FrontierMode::kDataOwner : FrontierMode::kDataAllReduce;
  }
  // in-kernel xGMI exchange of the owner histogram chunks, per-child bests or votes; else collectives
  p.try_xgmi = (env.dp_transport == DpTransport::kAuto || env.dp_transport == DpTransport::kXgmi) &&
               in.dp_ranks <= kMaxXRanks && frontier && !serial && p.frontier != FrontierMode::kDataAllReduce;
  p.xgmi_required = p.try_xgmi && env.dp_transport == DpTransport::kXgmi;
  // KNOWN: the voting frontier's extra-trees redraws are verified over
  // the in-kernel exchange only, so this combination aborts when the xGMI set-up fails at run time
  // (or is not tried: more than kMaxXRanks ranks) instead of taking the host policy.
  p.xgmi_needed = p.frontier == FrontierMode::kVoting && extra;

  // ---- the host split policy, by the learner type as configured (LGAP_FORCE_DEVICE_DP moves nothing)
  const bool type_serial = type == "serial", voting_extra = type == "voting" && extra;
  // One fp64 (g, h) histogram per open leaf, 2 x 8 bytes per bin: when num_leaves of them exceed
  // half of the device memory, the host learner's LRU pool bounds the live histograms within the
  // same budget. (histogram_pool_size stays a bound on the HOST cache: it moves nothing here.)
  const double mib = 1024.0 * 1024.0;
  const double budget = env.hist_budget_set ? env.hist_budget_mb * mib : 0.5 * static_cast<double>(in.device_total_memory);
  const bool exceeds_pool =
      d.has_data && budget > 0 && 16.0 * std::max(1, d.total_bins) * std::max(2, c->num_leaves) > budget;
  // what only the frontier implements on the device, on the serial learner as configured
  const bool serves = type_serial && !bynode && !extra && shape_fits(feature_pens, false);
  const bool serves_bynode = type_serial && !extra && shape_fits(true, false);
  const bool serves_mono = type_serial && !bynode && !extra && !forced_splits && !CegbPenalty::Enabled(c) &&
                           p.mono_inter && shape_fits(false, true);
  const bool frontier_ok = serves && (!feature_pens || ((!d.has_data || d.features <= 8192) && sets == 0));
  // linear leaves on the device (fp64 MFMA Gram systems): serial learner, float gradients, raw values
  // kept, at most kLinMaxM - 1 = 62 branch features per leaf (bounded by features, leaves and depth)
  long long branch = std::min<long long>(d.features, std::max(1, c->num_leaves) - 1);
  if (c->max_depth > 0) branch = std::min<long long>(branch, c->max_depth);
  const bool linear_on_device = type_serial && !c->use_quantized_grad && d.has_raw && branch + 1 <= kLinMaxM;
  if (exceeds_pool) {
    p.host_reason = "per-leaf device histograms above the histogram pool";
  } else if (in.linear_tree && !linear_on_device) {
    p.host_reason = "linear_tree";
  } else if (voting_extra && env.dp_transport != DpTransport::kXgmi &&
             (env.dp_transport != DpTransport::kAuto || env.device_dp_host)) {
    // (the host-staged / RCCL path of this combination is not tree-equal to the host)
    p.host_reason = "voting-parallel with extra_trees over collectives";
  } else if (voting_extra && CegbPenalty::Enabled(c)) {
    // (the device and host voting learners part after a few trees: not verified tree-equal)
    p.host_reason = "voting-parallel with extra_trees and CEGB";
  } else if (voting_extra && d.has_categorical) {
    p.host_reason = "voting-parallel with extra_trees and categorical features";
  } else if (feature_pens && !frontier_ok) {
    // (feature penalties and forced splits: the frontier's select only; the split penalty: every scan)
    p.host_reason = "cost-effective gradient boosting (feature penalties)";
  } else if (forced_splits && !frontier_ok) {
    p.host_reason = "forced splits";
  } else if (mono && (in.linear_tree || !serves_mono)) {
    // (intermediate: the frontier select walks the constraints and re-scans; advanced: the host walk)
    p.host_reason = "intermediate/advanced monotone constraints (device scans, host constraint walk)";
  } else if (sets > 0 && ((bynode && !serves_bynode) || (sets > 64 && !serves))) {
    // (the frontier holds 256 sets, the sequential chain 64; by-node masks over a node's allowed
    // pool are drawn in the frontier's select)
    p.host_reason = "interaction constraints with by-node sampling / more than 64 sets off the frontier";
  }
  if (p.host_reason != nullptr) {
    // the serial host learner's monotone constraint walk scans on the device (policy_scan.h);
    // extra-trees draws (which read the host histogram) and forced splits keep the host scans
    p.device_scans = type_serial && !in.linear_tree && mono && !extra && !forced_splits && !exceeds_pool;
    if (exceeds_pool && c->histogram_pool_size <= 0) {
      p.pool_budget_mb = env.hist_budget_set ? env.hist_budget_mb : 0.5 * static_cast<double>(in.device_total_memory) / mib;
    }
  }
  p.engine = p.host_reason != nullptr ? Engine::kHostPolicy : frontier ? Engine::kFrontier : Engine::kSequential;
  return p;
}

}  // namespace device
}  // namespace lgap
