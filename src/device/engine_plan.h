// Which engine trains a device_type=gpu configuration, decided in one place: the host split
// policy over HIP histograms, the device learner's frontier engine, or its sequential chain.
// PlanEngine is a pure function of PlanInputs (no HIP, no getenv): TreeLearner::Create asks it
// where to route, DeviceTreeLearner asks it again in Init / ResetConfig and branches on the answer.
// Its host_reason strings are the list of what the device learner does not serve.
#pragma once

#include <string>

#include "lgap/config.h"
#include "lgap/dataset.h"

namespace lgap {
namespace device {

// What the decision reads of the training data. has_data = false: no data yet (the frontier's
// shape is then judged by a conservative bound on num_leaves alone).
struct DataShape {
  bool has_data = false;
  int total_bins = 0, features = 0;   // Dataset::num_total_bin, inner (used) features
  int max_bin = 2, max_cat_bin = 1;   // widest feature, widest categorical feature
  bool has_categorical = false;
  bool has_raw = false;               // raw values kept (linear_tree)
};
DataShape ShapeOf(const Dataset* train);

// The environment knobs that move a configuration between engines. ReadRoutingEnv is their only
// reader; it runs with TreeLearner::Create and DeviceTreeLearner::Init / ResetConfig, never at
// process start (tests change the environment between trainings in one process). HostStagedDP()
// keeps its own cached read of LGAP_DEVICE_DP_TRANSPORT: it gates every collective, not routing.
enum class DpTransport { kAuto, kXgmi, kCollective, kAllreduce, kOther };
enum class ForceDP { kOff, kData, kVoting };
struct RoutingEnv {
  bool frontier_off = false;     // LGAP_FRONTIER=0: the sequential chain (A/B runs)
  bool frontier_dp_off = false;  // LGAP_FRONTIER_DP=0: the sequential owner-scan chain (A/B runs)
  DpTransport dp_transport = DpTransport::kAuto;  // LGAP_DP_TRANSPORT
  std::string dp_transport_text = "auto";         // (its value, for the error message of kOther)
  bool device_dp_host = false;   // LGAP_DEVICE_DP_TRANSPORT=host
  bool hist_budget_set = false;  // LGAP_DEVICE_HIST_BUDGET_MB: a smaller device budget (tests of the pooled route)
  double hist_budget_mb = 0.0;
  // LGAP_FORCE_DEVICE_DP=1 | voting: the data- / voting-parallel path on a one-rank communicator
  // (the configuration sets tree_learner to serial for one machine, as the reference does)
  ForceDP force_dp = ForceDP::kOff;
};
RoutingEnv ReadRoutingEnv();

struct PlanInputs {
  std::string learner_type = "serial";  // tree_learner
  bool linear_tree = false;
  const Config* config = nullptr;
  DataShape shape;
  size_t device_total_memory = 0;
  RoutingEnv env;
  // an RCCL communicator exists / has several ranks; host-staged collectives; data-parallel ranks
  bool comm_exists = false, comm_active = false, host_staged = false;
  int dp_ranks = 1;
};
// The inputs as the running process sees them (device_learner.hip: reads the device runtime).
PlanInputs GatherPlanInputs(const std::string& learner_type, bool linear_tree, const Config* c, const Dataset* train);

enum class Engine { kHostPolicy, kFrontier, kSequential };
enum class ParallelMode { kSerial, kData, kFeature, kVoting };
// the frontier's exchange per round: none (one device), the all-reduce of every histogram, the
// owner-computes reduce-scatter + best-split gather, the voting election, the feature-parallel bests
enum class FrontierMode { kNone, kSerial, kDataAllReduce, kDataOwner, kVoting, kFeature };

struct EnginePlan {
  Engine engine = Engine::kSequential;
  const char* host_reason = nullptr;  // why the device learner does not serve it (nullptr: it does)
  bool device_scans = false;          // the serial host learner scans on the device
  double pool_budget_mb = -1.0;       // the host histogram pool's budget (< 0: leave it)
  // device learner: the resolved parallel mode (LGAP_FORCE_DEVICE_DP applied) and its flags
  ParallelMode mode = ParallelMode::kSerial;
  bool voting = false, owner_scan = false, distributed = false;
  // kNone: the sequential chain (set whatever `engine` says: the host policy's histogram backend)
  FrontierMode frontier = FrontierMode::kNone;
  // in the select: per-node raw candidates of every feature (CEGB feature penalties, by-node
  // sampling), intermediate monotone constraints, by-node masks drawn under interaction constraints
  bool raw_cands = false, cegb_coupled = false, cegb_lazy = false, mono_inter = false, bynode_on_device = false;
  // set up the in-kernel xGMI exchange; a failed set-up is fatal (LGAP_DP_TRANSPORT=xgmi asked for
  // it); the engine cannot run without it
  bool try_xgmi = false, xgmi_required = false, xgmi_needed = false;
};

EnginePlan PlanEngine(const PlanInputs& in);
const char* EngineName(Engine e);

}  // namespace device
}  // namespace lgap
