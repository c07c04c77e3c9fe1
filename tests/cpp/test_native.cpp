// Native unit / integration tests of the C++ core, the analogue of the reference's
// tests/cpp_tests (test_single_row.cpp, test_stream.cpp, test_serialize.cpp,
// test_common.cpp): plain asserts, no framework. Built by `make cpptest`
// (build/test_native) and `make asan` (build/asan/test_native, host code under
// AddressSanitizer + UBSan); tests/test_native.py runs whichever exist.
//
//   test_native <path to tests/data>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "device/engine_plan.h"
#include "device/traverse_pack.h"
#include "lgap/c_api.h"
#include "lgap/common.h"
#include "lgap/log.h"
#include "lgap/pointwise_metric.h"
#include "lgap/random.h"
#include "lgap/split_math.h"
#include "learner/leaf_constraints.h"

namespace {

int g_failures = 0;

#define EXPECT(cond)                                                              \
  do {                                                                            \
    if (!(cond)) {                                                                \
      std::fprintf(stderr, "%s:%d: EXPECT failed: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failures;                                                               \
    }                                                                             \
  } while (0)

#define CHECK_API(call) EXPECT((call) == 0)

std::vector<std::vector<double>> LoadTsv(const std::string& path, std::vector<float>* label) {
  std::ifstream in(path);
  std::string line;
  std::vector<std::vector<double>> rows;
  while (std::getline(in, line)) {
    std::stringstream ss(line);
    double v;
    std::vector<double> r;
    bool first = true;
    while (ss >> v) {
      if (first) label->push_back(static_cast<float>(v));
      else r.push_back(v);
      first = false;
    }
    if (!r.empty()) rows.push_back(r);
  }
  return rows;
}

void TestRandom() {
  // the reference LCG stream (random.h:101-111): x = 214013 x + 2531011
  lgap::Random r(7);
  unsigned x = 7u;
  for (int i = 0; i < 100; ++i) {
    x = 214013u * x + 2531011u;
    const float expect = static_cast<float>((x >> 16) & 0x7FFF) / 32768.0f;
    EXPECT(r.NextFloat() == expect);
  }
  lgap::Random s(3);
  const auto sample = s.Sample(100, 10);
  EXPECT(sample.size() == 10u);
  for (size_t i = 1; i < sample.size(); ++i) EXPECT(sample[i] > sample[i - 1]);
}

void TestCommon() {
  const auto parts = lgap::common::Split("a,b,,c", ',');
  EXPECT(parts.size() >= 3u);
  double d = 0.0;
  EXPECT(lgap::common::AtofOrDie("1.5e3") == 1500.0);
  (void)d;
  const std::vector<int> cats = {1, 5, 33, 64};
  const auto bits = lgap::common::ConstructBitset(cats.data(), static_cast<int>(cats.size()));
  EXPECT(bits.size() == 3u);
  EXPECT((bits[0] >> 1) & 1u);
  EXPECT((bits[0] >> 5) & 1u);
  EXPECT((bits[1] >> 1) & 1u);
  EXPECT((bits[2] >> 0) & 1u);
  EXPECT(!((bits[0] >> 2) & 1u));
}

void TestPointwiseMetric() {
  lgap::PwMetricParams p;
  p.kind = lgap::kPmBinLogloss;
  p.output = lgap::kOutSigmoid;
  p.sigmoid = 1.0;
  const double t = lgap::PmRowTerm(p, 1.0, 0.0, false, 1.0);
  EXPECT(std::fabs(t - std::log(2.0)) < 1e-12);
  p.kind = lgap::kPmL2;
  p.output = lgap::kOutIdentity;
  EXPECT(lgap::PmRowTerm(p, 2.0, 5.0, true, 0.5) == 4.5);
}

void TestTrainPredictRoundTrip(const std::string& data) {
  std::vector<float> y;
  const auto rows = LoadTsv(data + "/binary.test", &y);
  EXPECT(!rows.empty());
  if (rows.empty()) return;
  const int ncol = static_cast<int>(rows[0].size());
  DatasetHandle ds = nullptr;
  CHECK_API(LGBM_DatasetCreateFromFile((data + "/binary.train").c_str(), "max_bin=63 verbosity=-1", nullptr, &ds));
  int n = 0;
  CHECK_API(LGBM_DatasetGetNumData(ds, &n));
  EXPECT(n == 7000);
  BoosterHandle b = nullptr;
  CHECK_API(LGBM_BoosterCreate(ds, "objective=binary num_leaves=15 verbosity=-1 device_type=cpu", &b));
  int finished = 0;
  for (int it = 0; it < 20 && !finished; ++it) CHECK_API(LGBM_BoosterUpdateOneIter(b, &finished));

  // batch predictions vs single-row fast path (test_single_row.cpp)
  std::vector<double> flat;
  for (const auto& r : rows) flat.insert(flat.end(), r.begin(), r.end());
  const int nr = static_cast<int>(rows.size());
  std::vector<double> batch(nr);
  int64_t len = 0;
  CHECK_API(LGBM_BoosterPredictForMat(b, flat.data(), C_API_DTYPE_FLOAT64, nr, ncol, 1, C_API_PREDICT_NORMAL, 0, -1,
                                      "", &len, batch.data()));
  EXPECT(len == nr);
  FastConfigHandle fc = nullptr;
  CHECK_API(LGBM_BoosterPredictForMatSingleRowFastInit(b, C_API_PREDICT_NORMAL, 0, -1, C_API_DTYPE_FLOAT64, ncol, "",
                                                       &fc));
  for (int i = 0; i < nr; i += 37) {
    double out = 0.0;
    CHECK_API(LGBM_BoosterPredictForMatSingleRowFast(fc, rows[i].data(), &len, &out));
    EXPECT(std::fabs(out - batch[i]) < 1e-12);
  }
  CHECK_API(LGBM_FastConfigFree(fc));

  // model text round trip (test_serialize.cpp analogue for the model)
  int64_t need = 0;
  CHECK_API(LGBM_BoosterSaveModelToString(b, 0, -1, 0, 0, &need, nullptr));
  std::string text(static_cast<size_t>(need), '\0');
  CHECK_API(LGBM_BoosterSaveModelToString(b, 0, -1, 0, need, &need, &text[0]));
  BoosterHandle b2 = nullptr;
  int iters = 0;
  CHECK_API(LGBM_BoosterLoadModelFromString(text.c_str(), &iters, &b2));
  EXPECT(iters == 20);
  std::vector<double> again(nr);
  CHECK_API(LGBM_BoosterPredictForMat(b2, flat.data(), C_API_DTYPE_FLOAT64, nr, ncol, 1, C_API_PREDICT_NORMAL, 0, -1,
                                      "", &len, again.data()));
  for (int i = 0; i < nr; ++i) EXPECT(again[i] == batch[i]);
  double acc = 0.0;
  for (int i = 0; i < nr; ++i) acc += ((batch[i] > 0.5) == (y[i] > 0.5)) ? 1.0 : 0.0;
  EXPECT(acc / nr > 0.7);
  CHECK_API(LGBM_BoosterFree(b2));
  CHECK_API(LGBM_BoosterFree(b));

  // streaming push rows into a dataset created by reference (test_stream.cpp)
  DatasetHandle st = nullptr;
  CHECK_API(LGBM_DatasetCreateByReference(ds, nr, &st));
  const int half = nr / 2;
  CHECK_API(LGBM_DatasetPushRows(st, flat.data(), C_API_DTYPE_FLOAT64, half, ncol, 0));
  CHECK_API(LGBM_DatasetPushRows(st, flat.data() + static_cast<size_t>(half) * ncol, C_API_DTYPE_FLOAT64, nr - half,
                                 ncol, half));
  int sn = 0;
  CHECK_API(LGBM_DatasetGetNumData(st, &sn));
  EXPECT(sn == nr);
  CHECK_API(LGBM_DatasetFree(st));
  CHECK_API(LGBM_DatasetFree(ds));
}

// Errors raised inside OpenMP regions (parsing) must come back as -1 + LGBM_GetLastError,
// never std::terminate (reference utils/openmp_wrapper.h:80-131).
void TestParallelErrorsReturnMinusOne() {
  const std::string dir = "/tmp";
  const std::string bad_csv = dir + "/lgap_native_bad.csv";
  {
    std::ofstream f(bad_csv);
    for (int i = 0; i < 20000; ++i) {
      if (i == 12345) f << "1,2.5,oops,4\n";
      else f << (i % 2) << "," << i * 0.5 << "," << (i % 7) << "," << (i % 3) << "\n";
    }
  }
  DatasetHandle ds = nullptr;
  EXPECT(LGBM_DatasetCreateFromFile(bad_csv.c_str(), "verbosity=-1", nullptr, &ds) == -1);
  EXPECT(std::strstr(LGBM_GetLastError(), "oops") != nullptr);
  EXPECT(LGBM_DatasetCreateFromFile(bad_csv.c_str(), "verbosity=-1 two_round=true", nullptr, &ds) == -1);
  EXPECT(std::strstr(LGBM_GetLastError(), "oops") != nullptr);
  // a bad label token (label column parsed inside the same region)
  const std::string bad_label = dir + "/lgap_native_badlabel.csv";
  {
    std::ofstream f(bad_label);
    for (int i = 0; i < 20000; ++i) f << (i == 777 ? "yes" : (i % 2 ? "1" : "0")) << "," << i << "," << i % 5 << "\n";
  }
  EXPECT(LGBM_DatasetCreateFromFile(bad_label.c_str(), "verbosity=-1", nullptr, &ds) == -1);
  EXPECT(std::strstr(LGBM_GetLastError(), "yes") != nullptr);
  // a query file whose sizes do not add up to the row count
  const std::string good = dir + "/lgap_native_rank.csv";
  {
    std::ofstream f(good);
    for (int i = 0; i < 1000; ++i) f << (i % 3) << "," << i << "," << i % 5 << "\n";
    std::ofstream q(good + ".query");
    q << "500\n400\n";
  }
  EXPECT(LGBM_DatasetCreateFromFile(good.c_str(), "verbosity=-1", nullptr, &ds) == -1);
  EXPECT(std::strlen(LGBM_GetLastError()) > 0);
  std::remove(bad_csv.c_str());
  std::remove(bad_label.c_str());
  std::remove(good.c_str());
  std::remove((good + ".query").c_str());
}

}  // namespace

// Piecewise per-bin bounds of the advanced monotone method against a dense per-bin
// model (reference monotone_constraints.hpp:872-965 UpdateConstraints semantics:
// a leaf output tightens the bound on the bin range [b, e) it shares).
void TestBinPiecesMatchDenseBounds() {
  lgap::Random r(7);
  for (int trial = 0; trial < 400; ++trial) {
    const int nb = 2 + r.NextShort(0, 60);
    const bool raise = trial & 1;
    lgap::BinPieces p;
    p.Reset(raise ? -INFINITY : INFINITY);
    std::vector<double> dense(nb, raise ? -INFINITY : INFINITY);
    for (int op = 0; op < 12; ++op) {
      const double v = r.NextShort(-8, 8) * 0.25;
      if (r.NextShort(0, 5) == 0) {
        p.TightenAll(v, raise);
        for (double& x : dense) x = raise ? std::max(x, v) : std::min(x, v);
        continue;
      }
      const uint32_t b = r.NextShort(0, nb), e = b + 1 + r.NextShort(0, nb);
      p.TightenRange(v, raise, b, e, nb);
      for (uint32_t t = b; t < std::min<uint32_t>(e, nb); ++t) dense[t] = raise ? std::max(dense[t], v) : std::min(dense[t], v);
    }
    std::vector<double> got(nb);
    p.Expand(nb, got.data());
    for (int t = 0; t < nb; ++t) EXPECT(got[t] == dense[t]);
    EXPECT(p.start[0] == 0);
    for (size_t i = 1; i < p.size(); ++i) EXPECT(p.start[i] > p.start[i - 1] && p.val[i] != p.val[i - 1]);
  }
}

// Engine routing table (device/engine_plan.h). Every row's expectation was recorded from the
// commit before the planner, whose three copies of the decision it replaced: the factory-level
// columns (host reason, device scans, pool budget) from that commit's HostPolicyReason /
// DeviceScansServe / FrontierServes* run on the same inputs, the learner-level columns (engine,
// exchange, xGMI) by reading DeviceTreeLearner there; `src` cites those lines of that commit's
// device_learner.hip. Base shape: 28 numerical features of 255 bins, 63 leaves, a 288 GB device.
struct PlanWant {
  lgap::device::Engine engine;
  lgap::device::FrontierMode frontier;  // compared on the device engines
  const char* reason = nullptr;
  bool scans = false;
  double budget = -1.0;
  bool try_xgmi = false, xgmi_required = false, xgmi_needed = false;
  bool raw = false, mono = false, byn_dev = false;
  lgap::device::ParallelMode mode = lgap::device::ParallelMode::kSerial;
};

struct PlanCase {
  lgap::Config config;
  lgap::device::PlanInputs in;
  PlanCase(const char* learner, const std::string& params) {
    const bool leaves = params.find("num_leaves") != std::string::npos;
    config.Set(lgap::Config::Str2Map(((leaves ? "verbosity=-1 " : "verbosity=-1 num_leaves=63 ") + params).c_str()));
    in.learner_type = learner;
    in.linear_tree = config.linear_tree;
    in.shape.has_data = true;
    Features(28);
    in.device_total_memory = 288ull << 30;
  }
  PlanCase& Features(int f) {
    in.shape.features = f;
    in.shape.total_bins = f * 255;
    in.shape.max_bin = 255;
    return *this;
  }
  // a communicator of `ranks` ranks
  PlanCase& Comm(int ranks) {
    in.comm_exists = true;
    in.comm_active = ranks > 1;
    in.dp_ranks = ranks;
    return *this;
  }
  PlanCase& Transport(lgap::device::DpTransport t) {
    in.env.dp_transport = t;
    return *this;
  }
};

template <typename Check>
void PlanCases(Check check) {
  using namespace lgap::device;  // NOLINT
  const Engine kHost = Engine::kHostPolicy, kFront = Engine::kFrontier, kSeq = Engine::kSequential;
  const FrontierMode kNone = FrontierMode::kNone;
  const char* kWhyForced = "forced splits";
  const char* kWhyCegb = "cost-effective gradient boosting (feature penalties)";
  const char* kWhyMono = "intermediate/advanced monotone constraints (device scans, host constraint walk)";
  const char* kWhyIc = "interaction constraints with by-node sampling / more than 64 sets off the frontier";
  const char* kWhyVoteColl = "voting-parallel with extra_trees over collectives";
  std::string sets65, sets257, pens28;
  for (int i = 0; i < 257; ++i) {
    const std::string s = std::string(i ? "," : "") + "[" + std::to_string(i % 28) + "," + std::to_string((i + 1) % 28) + "]";
    if (i < 65) sets65 += s;
    sets257 += s;
  }
  for (int i = 0; i < 28; ++i) pens28 += std::string(i ? "," : "") + "0.5";
  const std::string forced = "forcedsplits_filename=forced.json", coupled = "cegb_penalty_feature_coupled=" + pens28;
  const std::string inter = "monotone_constraints=1,-1,0 monotone_constraints_method=intermediate";
  const std::string advanced = "monotone_constraints=1,-1,0 monotone_constraints_method=advanced";
  auto want = [](Engine e, FrontierMode f) {
    PlanWant w;
    w.engine = e;
    w.frontier = f;
    return w;
  };
  auto host = [&](const char* why) {
    PlanWant w = want(kHost, kNone);
    w.reason = why;
    return w;
  };

  // ---- serial (src :1730-1742 FrontierEligible, :1759 FrontierSerial)
  check(1, PlanCase("serial", ""), want(kFront, FrontierMode::kSerial));
  {
    PlanCase c("serial", "");
    c.in.env.frontier_off = true;  // src :207
    check(2, c, want(kSeq, kNone));
  }
  // node capacity 4 L + 128 = 4128 > 4096 (src :186-190, :210)
  check(3, PlanCase("serial", "num_leaves=1000"), want(kSeq, kNone));
  check(4, PlanCase("serial", "extra_trees=true"), want(kFront, FrontierMode::kSerial));  // src :1734
  {
    PlanWant w = want(kFront, FrontierMode::kSerial);
    w.raw = true;  // src :1745
    check(5, PlanCase("serial", "feature_fraction_bynode=0.5"), w);
  }

  // ---- linear leaves (parent LinearOnDevice, src :4446-4453)
  {
    PlanCase c("serial", "linear_tree=true num_leaves=31");
    c.in.shape.has_raw = true;
    check(6, c, want(kFront, FrontierMode::kSerial));
    c.in.shape.has_raw = false;
    check(7, c, host("linear_tree"));
  }
  {
    PlanCase c("serial", "linear_tree=true num_leaves=127");
    c.Features(100).in.shape.has_raw = true;
    check(8, c, host("linear_tree"));  // min(100, 126) + 1 > 63
    PlanCase d("serial", "linear_tree=true num_leaves=127 max_depth=6");
    d.Features(100).in.shape.has_raw = true;
    check(9, d, want(kFront, FrontierMode::kSerial));
  }

  // ---- forced splits (parent FrontierServes, src :4470-4474)
  check(10, PlanCase("serial", forced), want(kFront, FrontierMode::kSerial));
  check(11, PlanCase("serial", forced + " feature_fraction_bynode=0.5"), host(kWhyForced));
  {
    PlanCase c("serial", forced);
    c.in.env.frontier_off = true;
    check(12, c, host(kWhyForced));
  }
  check(13, PlanCase("data", forced).Comm(8), host(kWhyForced));

  // ---- CEGB feature penalties
  {
    PlanWant w = want(kFront, FrontierMode::kSerial);
    w.raw = true;  // src :1745, :1758
    check(14, PlanCase("serial", coupled), w);
  }
  check(15, PlanCase("serial", coupled + " interaction_constraints=[0,1],[2,3]"), host(kWhyCegb));
  check(16, PlanCase("serial", coupled).Features(8193), host(kWhyCegb));
  check(17, PlanCase("data", coupled).Comm(8), host(kWhyCegb));

  // ---- monotone constraints (parent FrontierServesMonoInter, src :4476-4481; DeviceScansServe)
  {
    PlanWant w = want(kFront, FrontierMode::kSerial);
    w.mono = true;  // src :1748
    check(18, PlanCase("serial", inter), w);
  }
  check(19, PlanCase("serial", inter + " extra_trees=true"), host(kWhyMono));
  {
    PlanWant w = host(kWhyMono);
    w.scans = true;
    check(20, PlanCase("serial", advanced), w);
  }
  check(21, PlanCase("serial", advanced + " " + forced), host(kWhyMono));

  // ---- interaction constraints (parent FrontierServesByNode, src :4483-4486)
  check(22, PlanCase("serial", "interaction_constraints=" + sets65), want(kFront, FrontierMode::kSerial));
  check(23, PlanCase("serial", "interaction_constraints=" + sets257), host(kWhyIc));
  {
    PlanWant w = want(kFront, FrontierMode::kSerial);
    w.raw = w.byn_dev = true;  // src :1752
    check(24, PlanCase("serial", "interaction_constraints=[0,1],[2,3] feature_fraction_bynode=0.5"), w);
  }
  check(25, PlanCase("data", "interaction_constraints=[0,1],[2,3] feature_fraction_bynode=0.5").Comm(8), host(kWhyIc));

  // ---- data parallel over a communicator (src :1774-1795 FrontierDP / FrontierOwner, :371-396 SetupTransport)
  {
    PlanWant w = want(kFront, FrontierMode::kDataOwner);
    w.mode = ParallelMode::kData;
    w.try_xgmi = true;
    check(26, PlanCase("data", "").Comm(8), w);
    w.try_xgmi = false;
    check(28, PlanCase("data", "").Comm(8).Transport(DpTransport::kCollective), w);
    check(32, PlanCase("data", "").Comm(17), w);  // src :383, more than kMaxXRanks
    w.frontier = FrontierMode::kDataAllReduce;    // src :1794
    check(27, PlanCase("data", "").Comm(8).Transport(DpTransport::kAllreduce), w);
    w = want(kSeq, kNone);
    w.mode = ParallelMode::kData;
    PlanCase c("data", "");
    c.Comm(8).in.env.frontier_dp_off = true;  // src :1776
    check(29, c, w);
    check(30, PlanCase("data", "extra_trees=true").Comm(8), w);  // src :1734
    w.raw = true;
    check(31, PlanCase("data", "feature_fraction_bynode=0.5").Comm(8), w);  // src :1737
  }

  // ---- voting parallel over a communicator (src :1801-1803 FrontierVoting)
  {
    PlanWant w = want(kFront, FrontierMode::kVoting);
    w.mode = ParallelMode::kVoting;
    w.try_xgmi = true;
    check(33, PlanCase("voting", "").Comm(8), w);
    check(34, PlanCase("voting", "extra_trees=true").Comm(8).Transport(DpTransport::kCollective), host(kWhyVoteColl));
    PlanCase c("voting", "extra_trees=true");
    c.Comm(8).in.env.device_dp_host = true;
    check(35, c, host(kWhyVoteColl));
    // KNOWN: the engine needs xGMI, a failed set-up at run time is
    // fatal (src :389-391) where the host policy could have served it
    w.xgmi_required = w.xgmi_needed = true;
    check(36, c.Transport(DpTransport::kXgmi), w);
    PlanCase d("voting", "extra_trees=true");
    d.Comm(8).in.shape.has_categorical = true;
    d.in.shape.max_cat_bin = 16;
    check(37, d, host("voting-parallel with extra_trees and categorical features"));
    check(38, PlanCase("voting", "extra_trees=true cegb_penalty_split=0.1").Comm(8),
          host("voting-parallel with extra_trees and CEGB"));
    // KNOWN: the frontier cannot hold 1,000 leaves, so voting with a CEGB
    // split penalty grows on the sequential chain, whose vote scan never subtracts the penalty
    w = want(kSeq, kNone);
    w.mode = ParallelMode::kVoting;
    check(39, PlanCase("voting", "cegb_penalty_split=0.1 num_leaves=1000").Comm(8), w);
    // KNOWN (the same finding): numerical extra_trees there, whose vote scan never redraws
    check(42, PlanCase("voting", "extra_trees=true num_leaves=1000").Comm(8), w);
  }

  // ---- LGAP_FORCE_DEVICE_DP on a one-rank communicator (src :257-268)
  {
    PlanCase c("serial", "");
    c.Comm(1).in.env.force_dp = ForceDP::kData;
    PlanWant w = want(kFront, FrontierMode::kDataOwner);
    w.mode = ParallelMode::kData;
    w.try_xgmi = true;
    check(40, c, w);
    c.in.env.force_dp = ForceDP::kVoting;
    w.frontier = FrontierMode::kVoting;
    w.mode = ParallelMode::kVoting;
    check(40, c, w);
  }
  // ---- LGAP_DEVICE_HIST_BUDGET_MB=1 at 255 leaves: 16 B x 7,140 bins x 255 leaves = 29 MB
  {
    PlanCase c("serial", "num_leaves=255");
    c.in.env.hist_budget_set = true;
    c.in.env.hist_budget_mb = 1.0;
    PlanWant w = host("per-leaf device histograms above the histogram pool");
    w.budget = 1.0;
    check(41, c, w);
  }
}

// The planner against the table: no Dataset, no device.
void TestEnginePlan() {
  using namespace lgap::device;  // NOLINT
  int rows = 0;
  const lgap::LogLevel level = lgap::Log::Level();  // (the rows' configurations set verbosity=-1)
  PlanCases([&](int row, const PlanCase& c, const PlanWant& w) {
    PlanInputs in = c.in;
    in.config = &c.config;
    const EnginePlan p = PlanEngine(in);
    const int before = g_failures;
    EXPECT(p.engine == w.engine);
    EXPECT((p.host_reason == nullptr) == (w.reason == nullptr));
    if (p.host_reason != nullptr && w.reason != nullptr) EXPECT(std::string(p.host_reason) == w.reason);
    EXPECT(p.device_scans == w.scans);
    EXPECT(p.pool_budget_mb == w.budget);
    if (w.engine != Engine::kHostPolicy) {
      EXPECT(p.frontier == w.frontier);
      EXPECT(p.mode == w.mode);
      EXPECT(p.try_xgmi == w.try_xgmi && p.xgmi_required == w.xgmi_required && p.xgmi_needed == w.xgmi_needed);
      EXPECT(p.raw_cands == w.raw && p.mono_inter == w.mono && p.bynode_on_device == w.byn_dev);
    }
    if (g_failures != before) std::fprintf(stderr, "  ^ engine plan row %d\n", row);
    ++rows;
  });
  EXPECT(rows == 43);
  lgap::Log::ResetLevel(level);
}

// A child that holds no hessian is no split candidate even with min_sum_hessian_in_leaf = 0 and
// a count estimate that leaves it a row (split_math.h MinChildHessian): bins 0-3 are empty, the
// per-bin count estimates of bins 4-7 round to 9 of the 10 rows, the total absorbs its
// 2 * kEpsilon, and the leaf's gradient sum carries a residue.
void TestScanSkipsChildWithoutHessian() {
  lgap::SplitParams p;
  p.min_sum_hessian_in_leaf = 0.0;
  p.min_data_in_leaf = 1;
  lgap::FeatureScanMeta m;
  m.num_bin = 8;
  const double h[4] = {2.8, 32.4, 32.4, 32.4}, g[4] = {1.5, -20.0, 5.0, 12.0};
  double hist[16] = {0.0};
  double sum_g = 1e-5, sum_h = 0.0;
  for (int b = 3; b >= 0; --b) {  // (summed as the reverse pass does: the same bits)
    hist[2 * (4 + b)] = g[b];
    hist[2 * (4 + b) + 1] = h[b];
    sum_g += g[b];
    sum_h += h[b];
  }
  EXPECT(sum_h + 2 * lgap::kEpsilon == sum_h && lgap::kEpsilon + h[3] == h[3]);
  // the empty side comes out as exactly 0, and as one and three ulps of the total
  const double totals[3] = {sum_h, std::nextafter(sum_h, 1e9), std::nextafter(std::nextafter(std::nextafter(sum_h, 1e9), 1e9), 1e9)};
  for (const double total : totals) {
    lgap::SplitInfo out;
    out.Reset();
    const bool splittable = lgap::FindBestNumerical(hist, m, p, sum_g, total, 10, 0.0, lgap::LeafBounds(), &out);
    EXPECT(splittable);
    EXPECT(std::isfinite(out.gain) && out.gain > 0.0 && out.gain < 100.0);
    EXPECT(out.threshold >= 4u && out.threshold <= 6u);
    EXPECT(out.left_sum_hessian > 1.0 && out.right_sum_hessian > 1.0);
  }
}

// GradientQuantizer::Quantize under deterministic rounding against the levels' definition
// (tests/quantize_cases.py holds the same formulas for the device kernels): with mg = max |g|,
// gs = mg / (bins / 2), hs = mh / bins, the level of g is sign(g) * floor(|g * (1 / gs)| + 0.5)
// and the value returned float(level * gs); h likewise. g levels lie in [-bins / 2, bins / 2] and
// h levels in [0, bins], so 254 bins need levels wider than int8.
void TestGradientQuantizerLevels() {
  const int n = 1001;
  for (const int bins : {4, 5, 16, 254}) {
    for (const int pos : {0, n / 2, n - 1}) {
      lgap::Random rng(bins * 31 + pos);
      std::vector<float> g(n), h(n), qg(n), qh(n);
      for (int i = 0; i < n; ++i) {
        const float p = 0.02f + 0.96f * rng.NextFloat();
        g[i] = p - (rng.NextFloat() < 0.5f ? 1.f : 0.f);
        h[i] = p * (1.f - p);
      }
      g[pos] = pos == 0 ? -1.5f : 1.5f;  // the maxima, at the row under test
      h[pos] = 0.3f;
      lgap::GradientQuantizer q;
      q.Init(n, bins, 7, false);
      q.Quantize(g.data(), h.data(), n, false, qg.data(), qh.data());
      const double mg = static_cast<double>(1.5f), mh = static_cast<double>(0.3f);
      const double gs = mg / (bins / 2), hs = mh / bins;
      EXPECT(q.grad_scale() == gs && q.hess_scale() == hs);
      const int before = g_failures;
      int lo_g = 0, hi_g = 0, hi_h = 0;
      for (int i = 0; i < n; ++i) {
        const double xg = static_cast<double>(g[i]) * (1.0 / gs), xh = static_cast<double>(h[i]) * (1.0 / hs);
        const int lg = static_cast<int>(std::floor(std::fabs(xg) + 0.5)) * (g[i] < 0.f ? -1 : 1);
        const int lh = static_cast<int>(std::floor(xh + 0.5));
        EXPECT(lg >= -(bins / 2) && lg <= bins / 2);
        EXPECT(lh >= 0 && lh <= bins);
        EXPECT(qg[i] == static_cast<float>(lg * gs));
        EXPECT(qh[i] == static_cast<float>(lh * hs));
        // the host's own levels, recovered from what it returned
        EXPECT(std::lround(qg[i] / gs) == lg && std::lround(qh[i] / hs) == lh);
        lo_g = std::min(lo_g, lg);
        hi_g = std::max(hi_g, lg);
        hi_h = std::max(hi_h, lh);
        if (g_failures - before > 8) break;
      }
      if (g_failures != before) {
        std::fprintf(stderr, "  ^ gradient quantizer, %d bins, maxima at row %d\n", bins, pos);
        continue;
      }
      EXPECT((pos == 0 ? lo_g == -(bins / 2) : hi_g == bins / 2) && hi_h == bins);  // the extreme levels occur
    }
  }
}

// PackCompactNode (device/traverse_pack.h) against the decision on the decoded bin, for every
// group bin of every small feature shape. The packed decision is traverse_kernels.h's contract:
// outside [lo, hi] `out_left`, at gmiss `default_left`, otherwise gb <= tg. The decoded decision
// is GoLeft of split_scan.h (which the partition uses): the feature bin is the mfb outside the
// stored range, else local < mfb ? local : local + 1; the missing bin of the node's missing type
// takes `default_left`, every other bin goes left when it is <= the threshold.
void TestCompactNodePredicate() {
  using namespace lgap::device;  // NOLINT
  long long cases = 0;
  for (const int offset : {1, 5, 200}) {
    for (int nb = 2; nb <= 10; ++nb) {
      for (int mfb = 0; mfb < nb; ++mfb) {
        for (int dbin = 0; dbin < nb; ++dbin) {
          lgap::FeatureInfo fi;
          fi.group = 3;
          fi.offset = offset;
          fi.num_bin = nb;
          fi.mfb = static_cast<uint32_t>(mfb);
          fi.default_bin = static_cast<uint32_t>(dbin);
          for (int missing = 0; missing <= 2; ++missing) {
            for (int dleft = 0; dleft <= 1; ++dleft) {
              for (int thr = 0; thr < nb; ++thr) {
                const int8_t dt = static_cast<int8_t>((dleft ? lgap::kDefaultLeftMask : 0) | (missing << 2));
                TNode d;
                TCat c;
                PackCompactNode(fi, dt, thr, 7, ~4, 0, 0, &d, &c);
                const int before = g_failures;
                EXPECT(d.group == 3 && d.left == 7 && d.right == ~4 && (d.flags & kTCat) == 0);
                EXPECT(((d.flags & kTDefaultLeft) != 0) == (dleft != 0));
                for (int gb = 0; gb < offset + nb + 3; ++gb, ++cases) {
                  bool packed;
                  if (gb < d.lo || gb > d.hi) packed = (d.flags & kTOutLeft) != 0;
                  else if (gb == d.gmiss) packed = (d.flags & kTDefaultLeft) != 0;
                  else packed = gb <= d.tg;
                  const int local = gb - offset;
                  const int b = (local < 0 || local >= nb - 1) ? mfb : (local < mfb ? local : local + 1);
                  const bool is_missing = (missing == 1 && b == dbin) || (missing == 2 && b == nb - 1);
                  const bool decoded = is_missing ? dleft != 0 : b <= thr;
                  EXPECT(packed == decoded);
                }
                if (g_failures != before) {
                  std::fprintf(stderr, "  ^ offset %d num_bin %d mfb %d default_bin %d missing %d default_left %d thr %d\n",
                               offset, nb, mfb, dbin, missing, dleft, thr);
                  if (g_failures > 50) return;
                }
              }
            }
          }
        }
      }
    }
  }
  EXPECT(cases > 4000000);  // (nothing skipped)

  // a categorical node: the flag, the feature's decode data and the word range
  {
    lgap::FeatureInfo fi;
    fi.group = 9;
    fi.offset = 17;
    fi.num_bin = 40;
    fi.mfb = 6;
    TNode d;
    TCat c;
    PackCompactNode(fi, lgap::kCategoricalMask, 2, ~0, 5, 11, 2, &d, &c);
    EXPECT(d.flags == kTCat && d.group == 9 && d.left == ~0 && d.right == 5 && d.gmiss == -1);
    EXPECT(c.offset == 17 && c.num_bin == 40 && c.mfb == 6 && c.begin == 11 && c.nwords == 2 && c.pad == 0);
  }

  // the staged layout: 256-byte aligned parts that add up, and the tree packed through it
  {
    lgap::Tree tree(32);
    const uint32_t bits[3] = {0x5u, 0x0u, 0x80000000u};
    for (int l = 0; l < 19; ++l) {
      if (l == 4) tree.SplitCategorical(l, 0, 0, bits, 3, bits, 3, 0.5, -0.5, 1, 1, 1.0, 1.0, 1.f, lgap::MissingType::None);
      else tree.Split(l, 0, 0, 1, 0.5, 0.25 * l, -0.25 * l, 1, 1, 1.0, 1.0, 1.f, lgap::MissingType::None, false);
    }
    const int nl = tree.num_leaves(), nn = nl - 1;
    EXPECT(nl == 20);
    const CompactLayout z = CompactTreeLayout(&tree);
    EXPECT(z.cat % 256 == 0 && z.leaf % 256 == 0 && z.bit % 256 == 0);
    EXPECT(z.cat >= sizeof(TNode) * nn && z.leaf - z.cat >= sizeof(TCat) * nn && z.bit - z.leaf >= sizeof(double) * nl);
    EXPECT(z.cat < sizeof(TNode) * nn + 256 && z.leaf - z.cat < sizeof(TCat) * nn + 256 &&
           z.bit - z.leaf < sizeof(double) * nl + 256);
    EXPECT(z.total == z.bit + sizeof(uint32_t) * tree.cat_threshold_inner().size());
    const CompactTreeDev t = CompactTreeAt(static_cast<const char*>(nullptr) + 4096, z, nl);
    EXPECT(reinterpret_cast<const char*>(t.cats) - reinterpret_cast<const char*>(t.nodes) == static_cast<long>(z.cat));
    EXPECT(reinterpret_cast<const char*>(t.leaf_value) - reinterpret_cast<const char*>(t.nodes) == static_cast<long>(z.leaf));
    EXPECT(reinterpret_cast<const char*>(t.cat_bits) - reinterpret_cast<const char*>(t.nodes) == static_cast<long>(z.bit));
    EXPECT(t.num_nodes == nn && t.num_leaves == nl);
  }
}

int main(int argc, char** argv) {
  const std::string data = argc > 1 ? argv[1] : "tests/data";
  TestEnginePlan();
  TestCompactNodePredicate();
  TestGradientQuantizerLevels();
  TestRandom();
  TestCommon();
  TestPointwiseMetric();
  TestScanSkipsChildWithoutHessian();
  TestTrainPredictRoundTrip(data);
  TestParallelErrorsReturnMinusOne();
  TestBinPiecesMatchDenseBounds();
  if (g_failures) {
    std::fprintf(stderr, "%d expectation(s) failed\n", g_failures);
    return 1;
  }
  std::printf("test_native: all passed\n");
  return 0;
}
