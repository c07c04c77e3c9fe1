// Fixed resources of the device engines, free of HIP headers: the limits and the LDS / capacity
// arithmetic shared by the kernels (frontier.h, tree_kernels.h, linear_kernels.h) and the engine
// planner (engine_plan.cpp, plain C++), so what the planner admits is what the kernels launch with.
#pragma once

#include <algorithm>
#include <cstddef>

#ifdef __HIPCC__
#define LGAP_HOST_DEVICE __host__ __device__
#else
#define LGAP_HOST_DEVICE
#endif

namespace lgap {
namespace device {

constexpr int kFrontierKmax = 64;        // expansions per round (compile-time cap)
constexpr int kFrontierMaxNodes = 4096;  // computed-node capacity of the select's LDS image
constexpr int kFrontierIcWords = 4;      // interaction-constraint sets on the frontier: 4 x 64
constexpr int kMaxXRanks = 16;           // xGMI transport: ranks of one node
constexpr int kLinMaxM = 63;             // linear leaves: unknowns per leaf, <= 62 branch features + the constant
constexpr size_t kFrontierLdsLimit = 150 * 1024;  // dynamic LDS one workgroup of the select / scan may take

// entries of the select's sort of the alive nodes: a power of two >= C (C <= kFrontierMaxNodes)
LGAP_HOST_DEVICE inline int FrontierSortCap(int C) {
  int p = 64;
  while (p < C) p <<= 1;
  return p;
}

// dynamic LDS of k_f_select (CEGB coupled penalties add F bytes of used flags after it)
LGAP_HOST_DEVICE inline size_t FrontierSelectLds(int C, int L) {
  return static_cast<size_t>(C) * (sizeof(double) + 6 * sizeof(int) + 1) + 64 +
         static_cast<size_t>(L) * (3 * sizeof(int) + sizeof(double) + sizeof(int)) + 64 +
         static_cast<size_t>(FrontierSortCap(C)) * (sizeof(double) + sizeof(int));
}

// extra LDS of the intermediate-monotone select (after FrontierSelectLds): per-leaf current and
// scan bounds, per-node thresholds, the committed node's ancestor levels, per-feature monotone
// types
LGAP_HOST_DEVICE inline size_t FrontierSelectMonoLds(int C, int L, int F) {
  return 16 + static_cast<size_t>(L) * (2 * 16 + 3 * sizeof(int) + 1) + static_cast<size_t>(C) * sizeof(int) +
         static_cast<size_t>(F) + 16;
}

// Computed-node capacity of one frontier tree: every committed node (2 L - 1) plus room for
// speculation (8 L + 2 kmax, fewer when the per-node fp64 histograms would exceed ~8 GiB).
inline int FrontierCapacityFor(int L, int TB) {
  const long long lo = 4LL * L + 2 * kFrontierKmax, hi = 8LL * L + 2 * kFrontierKmax;
  const long long slot_bytes = 16LL * std::max(TB, 1);
  const long long fit = (8LL << 30) / slot_bytes;
  const long long c = std::max(lo, std::min({hi, fit, static_cast<long long>(kFrontierMaxNodes)}));
  return static_cast<int>(c);
}

// LDS of the frontier's k_f_scan: two full fp64 (g, h) histograms of the widest feature plus
// the categorical sort arrays (index, ctr) of both scanning waves.
inline size_t FrontierScanLds(int max_bin, int max_cat_bin) {
  int cat_p2 = 1;
  while (cat_p2 < max_cat_bin) cat_p2 <<= 1;
  return static_cast<size_t>(max_bin) * 4 * sizeof(double) + static_cast<size_t>(cat_p2) * 2 * (sizeof(int) + sizeof(double));
}

}  // namespace device
}  // namespace lgap
