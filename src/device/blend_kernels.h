// Blended score updates: score[i] = blend(score[i], v_i) where the existing kernels do
// score[i] += v_i (ScoreBlend, lgap/tree_learner.h): divide ? (s * pre + v) / post
// : (s * pre + v) * post, three separately rounded fp64 operations, the bits of the host's three
// passes over the score in RF::TrainOneIter / RF::RollbackOneIter. Each kernel reads and writes
// the score once.
//
// blend_kernels.hip is built with -ffp-contract=off (Makefile): under the tree-wide
// -ffp-contract=fast the multiply and the add become one fused multiply-add whatever the source
// says, and a fused result does not have the host's bits. The walk itself (traverse_device.h) is
// the one k_traverse / k_traverse_col make; those kernels are not touched.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device/traverse_pack.h"
#include "lgap/tree_learner.h"

namespace lgap {
namespace device {

// k_traverse with the blend: width 0 = 4-bit rows, 1 = 8-bit, 2 = 16-bit group bins. grid_cap > 0
// caps the grid (tests: several tiles per block at small row counts).
void LaunchBlendTraverse(const uint32_t* rowbins, int stride_dw, int width, int n, const CompactTreeDev& t,
                         const ScoreBlend& b, double* score, int num_cu, int grid_cap, hipStream_t s);
// k_traverse_col with the blend: the group-major copy colbins[g * n + row] of wide training rows
void LaunchBlendTraverseCols(const uint8_t* colbins, int width, int n, const CompactTreeDev& t, const ScoreBlend& b,
                             double* score, int num_cu, int grid_cap, hipStream_t s);
// k_leaf_add with the blend: score[i] = blend(score[i], lv[map[i]]) (LaunchLeafMapAdd's map)
void LaunchBlendLeafMapAdd(const void* map, const double* lv, int num_leaves, int n, const ScoreBlend& b,
                           double* score, int num_cu, hipStream_t s);
// a one-leaf tree: score[i] = blend(score[i], v)
void LaunchBlendConstant(double* score, int n, double v, const ScoreBlend& b, hipStream_t s);
// score[i] = divide ? score[i] / f : score[i] * f (the unfused blend around a plain add)
void LaunchBlendScale(double* score, int n, double f, bool divide, hipStream_t s);

}  // namespace device
}  // namespace lgap
