// TreeLearner factory (reference src/treelearner/tree_learner.cpp:15-57).
// device_type=cpu -> host learners. device_type=gpu|cuda -> the device-resident
// HIP learner, or — when a split policy only the host learners implement is
// requested — the host learner of that type with HIP histograms (the
// reference's GPUTreeLearner arrangement). Fails loudly when no MI355X is
// visible: no silent CPU fallback.
#include "lgap/tree_learner.h"

#include <cstdlib>
#include <cstring>

#include "device/engine_plan.h"
#include "lgap/device_api.h"
#include "lgap/log.h"
#include "parallel_tree_learner.h"
#include "serial_tree_learner.h"

namespace lgap {

namespace {

std::unique_ptr<TreeLearner> CreateHost(const std::string& learner_type, bool linear_tree, const Config* config) {
  if (linear_tree) return CreateLinearTreeLearner(config);
  if (learner_type == "serial") return std::make_unique<SerialTreeLearner>(config);
  if (learner_type == "feature") return std::make_unique<FeatureParallelTreeLearner>(config);
  if (learner_type == "data") return std::make_unique<DataParallelTreeLearner>(config);
  if (learner_type == "voting") return std::make_unique<VotingParallelTreeLearner>(config);
  Log::Fatal("Unknown tree learner type %s", learner_type.c_str());
  return nullptr;
}

}  // namespace

DeviceDart DeviceDartMode() {
  static const DeviceDart mode = [] {
    const char* e = std::getenv("LGAP_DEVICE_DART");
    if (e == nullptr || std::strcmp(e, "tree") == 0) return DeviceDart::kTree;
    if (std::strcmp(e, "forest") == 0) return DeviceDart::kForest;
    if (std::strcmp(e, "0") == 0) return DeviceDart::kHost;
    Log::Fatal("LGAP_DEVICE_DART: unknown value '%s' (forest, tree or 0)", e);
    return DeviceDart::kTree;
  }();
  return mode;
}

bool DeviceRfMode() {
  static const bool device = [] {
    const char* e = std::getenv("LGAP_DEVICE_RF");
    if (e == nullptr || std::strcmp(e, "1") == 0) return true;
    if (std::strcmp(e, "0") == 0) return false;
    Log::Fatal("LGAP_DEVICE_RF: unknown value '%s' (1 or 0)", e);
    return true;
  }();
  return device;
}

// Only a learner that owns the score on the device serves these (the boosting loop refuses
// earlier, with the advice to use Booster.update; reaching them is a routing bug).
void TreeLearner::DeviceSetGradientsFromDevice(const DeviceGradView&) {
  Log::Fatal("This tree learner keeps its gradients on the host: pass host arrays through Booster.update(fobj=...)");
}
void TreeLearner::DeviceCopyScoreTo(int, double*, size_t) {
  Log::Fatal("This tree learner keeps its scores on the host: read them through Booster.update(fobj=...) / eval");
}
void TreeLearner::DeviceUploadScoreTo(const double*, double*, size_t) {
  Log::Fatal("This tree learner keeps its scores on the host: read them through Booster.update(fobj=...) / eval");
}

std::unique_ptr<TreeLearner> TreeLearner::Create(const std::string& learner_type, const std::string& device_type,
                                                 bool linear_tree, const Config* config, const Dataset* train) {
  if (device_type == "gpu" || device_type == "cuda") {
    if (device::DeviceCount() <= 0) {
      Log::Fatal("device_type=%s requested but no AMD GPU (gfx950) is visible to HIP", device_type.c_str());
    }
    // one decision for the factory and the device learner (device/engine_plan.h)
    const device::EnginePlan plan = device::PlanEngine(device::GatherPlanInputs(learner_type, linear_tree, config, train));
    if (plan.engine != device::Engine::kHostPolicy) return device::CreateDeviceTreeLearner(config, learner_type);
    Log::Info("%s: host split policy over HIP histograms", plan.host_reason);
    auto learner = CreateHost(learner_type, linear_tree, config);
    auto* serial = static_cast<SerialTreeLearner*>(learner.get());
    serial->EnableDeviceHistograms();
    if (plan.device_scans) serial->EnableDeviceScans();
    if (plan.pool_budget_mb >= 0) serial->SetHistPoolBudgetMB(plan.pool_budget_mb);
    return learner;
  }
  if (device_type != "cpu") Log::Fatal("Unknown device type %s", device_type.c_str());
  return CreateHost(learner_type, linear_tree, config);
}

}  // namespace lgap
