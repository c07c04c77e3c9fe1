// SHAP values on the device (Booster.predict_contrib_device): the launch plan of
// k_predict_contrib. The plan is plain host arithmetic, kept apart from the kernel so its
// thresholds are stated once.
#pragma once

#include <cstddef>
#include <cstdint>

#include "device/contrib_pack.h"

namespace lgap {
namespace device {

constexpr int kCMaxThreads = 256;          // one lane owns one row; a block's tile is its lane count
constexpr int kCMinThreads = 64;
constexpr int kCLdsBytes = 64 * 1024;      // dynamic LDS of one block: two blocks fit the CU's 160 KiB
constexpr int kCWeightLdsBytes = 34 * 1024;  // the lanes' weight arrays, (max_path + 1) doubles each

struct ContribShape {
  int threads;       // lanes (= rows) of a block: 256, 128 or 64
  int w_slots;       // max_path + 1
  int phi_lds;       // the tile's contributions are kept in LDS and written out coalesced
  int stage_rows;    // the tile's rows are staged in LDS
  size_t lds_bytes;  // dynamic LDS of the launch
};

// The largest block whose weight arrays ([slot][lane], 8 B x lanes x (max_path + 1)) fit
// kCWeightLdsBytes: 256 lanes up to 16 unique features per path, 128 up to 33, 64 up to
// kCMaxPathFeatures. Then, in what is left of kCLdsBytes, the contribution tile
// (8 B x lanes x width) if it fits, then the staged rows (lanes x ncol x elem) if they fit.
inline ContribShape PlanContribShape(int max_path, int width, int ncol, size_t elem) {
  ContribShape s{};
  s.w_slots = max_path + 1;
  s.threads = kCMaxThreads;
  while (s.threads > kCMinThreads &&
         sizeof(double) * static_cast<size_t>(s.threads) * s.w_slots > static_cast<size_t>(kCWeightLdsBytes)) {
    s.threads /= 2;
  }
  size_t used = sizeof(double) * static_cast<size_t>(s.threads) * s.w_slots;
  const size_t phi_bytes = sizeof(double) * static_cast<size_t>(s.threads) * static_cast<size_t>(width);
  s.phi_lds = used + phi_bytes <= static_cast<size_t>(kCLdsBytes) ? 1 : 0;
  if (s.phi_lds) used += phi_bytes;
  const size_t row_bytes = (static_cast<size_t>(s.threads) * ncol * elem + 15) & ~static_cast<size_t>(15);
  s.stage_rows = used + row_bytes <= static_cast<size_t>(kCLdsBytes) ? 1 : 0;
  if (s.stage_rows) used += row_bytes;
  s.lds_bytes = used;
  return s;
}

// nrow x ContribWidth doubles in out. `data` and `out` may each be host memory (moved in chunks
// of at most 256 MiB of the larger of input and output) or memory of the current device, used
// in place. The work is complete when the call returns. Fails without a GPU.
void PredictContribDense(const ContribPack& pack, const void* data, bool f64, int nrow, int ncol,
                         bool data_on_device, bool out_on_device, double* out);

}  // namespace device
}  // namespace lgap
