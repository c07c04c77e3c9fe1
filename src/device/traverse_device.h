// Device-side pieces every row-walk kernel shares (traverse_kernels.hip, blend_kernels.hip): the
// tile shape, the group-bin read of a packed row, one level of a walk, and the staging of a row
// tile into LDS. Header-only and force-inlined: each translation unit compiles its own copy under
// its own floating-point flags (none of this is floating-point code).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "device/traverse_pack.h"

namespace lgap {
namespace device {

constexpr int kTThreads = 256;
constexpr int kTRowsPerThread = 2;
constexpr int kTRows = kTThreads * kTRowsPerThread;
constexpr int kTMaxDw = 16;  // wider rows read global memory directly

// Row-walk grid: 8 blocks per CU, grid-stride over the chunks
inline int TraverseGrid(long long n, int num_cu) {
  const long long chunks = (n + kTRows - 1) / kTRows;
  return static_cast<int>(std::max<long long>(1, std::min<long long>(chunks, static_cast<long long>(num_cu) * 8)));
}

template <int W>
__device__ __forceinline__ uint32_t GroupBin(const uint8_t* row, int g) {
  if (W == 0) return (row[g >> 1] >> ((g & 1) * 4)) & 0xFu;  // 4-bit rows
  return W == 1 ? row[g] : reinterpret_cast<const uint16_t*>(row)[g];
}

__device__ __forceinline__ bool CatLeft(const TCat& c, const uint32_t* bits, uint32_t gb) {
  const int local = static_cast<int>(gb) - c.offset;
  uint32_t b;
  if (local < 0 || local >= c.num_bin - 1) b = static_cast<uint32_t>(c.mfb);
  else b = static_cast<uint32_t>(local < c.mfb ? local : local + 1);
  const uint32_t w = b >> 5;
  return static_cast<int>(w) < c.nwords && ((bits[c.begin + w] >> (b & 31u)) & 1u);
}

// One level of a walk: the child of node `node` (its packed form `nd`) that a row whose group bin
// is `gb` goes to (>= 0: a node, < 0: ~leaf). The group-bin predicate of traverse_kernels.h, the
// one copy every traversal kernel calls.
__device__ __forceinline__ int NodeStep(const TNode& nd, uint32_t gb, const TCat* __restrict__ cats,
                                        const uint32_t* __restrict__ cat_bits, int node) {
  bool left;
  if (nd.flags & kTCat) {
    left = CatLeft(cats[node], cat_bits, gb);
  } else if (gb < nd.lo || gb > nd.hi) {
    left = (nd.flags & kTOutLeft) != 0;
  } else if (static_cast<int>(gb) == nd.gmiss) {
    left = (nd.flags & kTDefaultLeft) != 0;
  } else {
    left = gb <= nd.tg;
  }
  return left ? nd.left : nd.right;
}

// A tile of `ndw` dwords of packed rows from `src` into LDS: 16-byte loads where the tile is
// 16-byte aligned (kTRows * stride_dw dwords per tile: always, for rows from a 16-byte aligned
// buffer), dword loads for the tail. The caller puts the barriers around it. k_traverse and
// k_traverse_forest keep the same lines written out: calling this from them reorders their
// instructions, and their compiled code is held fixed.
__device__ __forceinline__ void StageRowTile(const uint32_t* src, int ndw, uint32_t* s_rows, int t) {
  const int nq = (reinterpret_cast<uintptr_t>(src) & 15u) == 0 ? ndw >> 2 : 0;
  const uint4* src4 = reinterpret_cast<const uint4*>(src);
  uint4* dst4 = reinterpret_cast<uint4*>(s_rows);
  for (int k = t; k < nq; k += kTThreads) dst4[k] = src4[k];
  for (int k = 4 * nq + t; k < ndw; k += kTThreads) s_rows[k] = src[k];
}

}  // namespace device
}  // namespace lgap
