// Blended score updates (see blend_kernels.h). Built with -ffp-contract=off: Blend() below must
// stay a multiply, an add and a multiply (or a divide), each rounded on its own.
//
// Streaming kernels: the traversal variants are k_traverse / k_traverse_col (traverse_kernels.hip)
// with the last line changed, the same tile of kTRows rows per block, the same LDS layout (nodes,
// leaf values, the staged row tile) and grid; the leaf-add variant is k_leaf_add without its
// gradient half, 16-byte score accesses over four rows per lane.
#include "device/blend_kernels.h"

#include <algorithm>

#include "device/hip_common.h"
#include "device/traverse_device.h"
#include "device/traverse_kernels.h"
#include "lgap/log.h"

namespace lgap {
namespace device {
namespace {

__device__ __forceinline__ double Blend(double s, double v, const ScoreBlend& b) {
  const double t = s * b.pre + v;
  return b.divide ? t / b.post : t * b.post;
}

template <int W>
__global__ __launch_bounds__(kTThreads) void k_blend_traverse(const uint32_t* __restrict__ rowbins, int stride_dw, int n,
                                                              const TNode* __restrict__ nodes, int num_nodes,
                                                              const TCat* __restrict__ cats,
                                                              const uint32_t* __restrict__ cat_bits,
                                                              const double* __restrict__ leaf_value, int num_leaves,
                                                              double* __restrict__ score, ScoreBlend b) {
  extern __shared__ __align__(16) unsigned char lds[];
  TNode* s_nodes = reinterpret_cast<TNode*>(lds);
  double* s_leaf = reinterpret_cast<double*>(lds + ((sizeof(TNode) * num_nodes + 15) & ~size_t(15)));
  uint32_t* s_rows = reinterpret_cast<uint32_t*>(reinterpret_cast<unsigned char*>(s_leaf) +
                                                 ((sizeof(double) * num_leaves + 15) & ~size_t(15)));
  const int t = threadIdx.x;
  for (int i = t; i < num_nodes * static_cast<int>(sizeof(TNode) / 4); i += kTThreads) {
    reinterpret_cast<uint32_t*>(s_nodes)[i] = reinterpret_cast<const uint32_t*>(nodes)[i];
  }
  for (int i = t; i < num_leaves; i += kTThreads) s_leaf[i] = leaf_value[i];
  const bool staged = stride_dw <= kTMaxDw;
  for (long long base = static_cast<long long>(blockIdx.x) * kTRows; base < n;
       base += static_cast<long long>(gridDim.x) * kTRows) {
    const int rows = static_cast<int>(min(static_cast<long long>(kTRows), n - base));
    // this chunk's scores, loaded before the walk so their latency hides behind it
    double sc[kTRowsPerThread];
#pragma unroll
    for (int j = 0; j < kTRowsPerThread; ++j) {
      const int r = t + j * kTThreads;
      sc[j] = r < rows ? score[base + r] : 0.0;
    }
    if (staged) {
      __syncthreads();  // the previous chunk's walks are done (first pass: nodes / leaves in place)
      StageRowTile(rowbins + base * stride_dw, rows * stride_dw, s_rows, t);
      __syncthreads();
    } else if (base == static_cast<long long>(blockIdx.x) * kTRows) {
      __syncthreads();
    }
    const uint8_t* row[kTRowsPerThread];
    int node[kTRowsPerThread];
#pragma unroll
    for (int j = 0; j < kTRowsPerThread; ++j) {
      const int r = t + j * kTThreads;
      node[j] = r < rows ? 0 : ~0;
      row[j] = staged ? reinterpret_cast<const uint8_t*>(s_rows + static_cast<size_t>(r) * stride_dw)
                      : reinterpret_cast<const uint8_t*>(rowbins + static_cast<size_t>(base + r) * stride_dw);
    }
    bool live = true;
    while (live) {
      live = false;
#pragma unroll
      for (int j = 0; j < kTRowsPerThread; ++j) {
        if (node[j] < 0) continue;
        const TNode nd = s_nodes[node[j]];
        const uint32_t gb = GroupBin<W>(row[j], nd.group);
        node[j] = NodeStep(nd, gb, cats, cat_bits, node[j]);
        live |= node[j] >= 0;
      }
    }
#pragma unroll
    for (int j = 0; j < kTRowsPerThread; ++j) {
      const int r = t + j * kTThreads;
      if (r < rows) score[base + r] = Blend(sc[j], s_leaf[~node[j]], b);
    }
  }
}

template <int W>
__global__ __launch_bounds__(kTThreads) void k_blend_traverse_col(const uint8_t* __restrict__ colbins, int n,
                                                                  const TNode* __restrict__ nodes, int num_nodes,
                                                                  const TCat* __restrict__ cats,
                                                                  const uint32_t* __restrict__ cat_bits,
                                                                  const double* __restrict__ leaf_value, int num_leaves,
                                                                  double* __restrict__ score, ScoreBlend b) {
  extern __shared__ __align__(16) unsigned char lds[];
  TNode* s_nodes = reinterpret_cast<TNode*>(lds);
  double* s_leaf = reinterpret_cast<double*>(lds + ((sizeof(TNode) * num_nodes + 15) & ~size_t(15)));
  const int t = threadIdx.x;
  for (int i = t; i < num_nodes * static_cast<int>(sizeof(TNode) / 4); i += kTThreads) {
    reinterpret_cast<uint32_t*>(s_nodes)[i] = reinterpret_cast<const uint32_t*>(nodes)[i];
  }
  for (int i = t; i < num_leaves; i += kTThreads) s_leaf[i] = leaf_value[i];
  __syncthreads();
  for (long long base = static_cast<long long>(blockIdx.x) * kTRows; base < n;
       base += static_cast<long long>(gridDim.x) * kTRows) {
    long long row[kTRowsPerThread];
    int node[kTRowsPerThread];
    double sc[kTRowsPerThread];
#pragma unroll
    for (int j = 0; j < kTRowsPerThread; ++j) {
      row[j] = base + t + j * kTThreads;
      node[j] = row[j] < n ? 0 : ~0;
      sc[j] = row[j] < n ? score[row[j]] : 0.0;
    }
    bool live = true;
    while (live) {
      live = false;
#pragma unroll
      for (int j = 0; j < kTRowsPerThread; ++j) {
        if (node[j] < 0) continue;
        const TNode nd = s_nodes[node[j]];
        const size_t o = static_cast<size_t>(nd.group) * n + row[j];
        const uint32_t gb = W == 1 ? colbins[o] : reinterpret_cast<const uint16_t*>(colbins)[o];
        node[j] = NodeStep(nd, gb, cats, cat_bits, node[j]);
        live |= node[j] >= 0;
      }
    }
#pragma unroll
    for (int j = 0; j < kTRowsPerThread; ++j) {
      if (row[j] < n) score[row[j]] = Blend(sc[j], s_leaf[~node[j]], b);
    }
  }
}

constexpr int kBAThreads = 256;

// score[i] = blend(score[i], lv[map[i]]): four rows per lane where the score slice is 16-byte
// aligned (vec), else and for the tail one row per lane. Leaf values in LDS.
template <typename T>
__global__ __launch_bounds__(kBAThreads) void k_blend_leaf_add(const T* __restrict__ map,
                                                               const double* __restrict__ leaf_value, int nl, int n,
                                                               bool vec, double* __restrict__ score, ScoreBlend b) {
  __shared__ double s_lv[kLMMaxLeaves];
  for (int i = threadIdx.x; i < nl; i += kBAThreads) s_lv[i] = leaf_value[i];
  __syncthreads();
  const int stride = gridDim.x * kBAThreads;
  const int quads = vec ? n >> 2 : 0;
  for (int q = blockIdx.x * kBAThreads + threadIdx.x; q < quads; q += stride) {
    uint32_t l[4];
    if (sizeof(T) == 1) {
      const uint32_t m = reinterpret_cast<const uint32_t*>(map)[q];
      l[0] = m & 0xFFu, l[1] = (m >> 8) & 0xFFu, l[2] = (m >> 16) & 0xFFu, l[3] = m >> 24;
    } else {
      const uint2 m = reinterpret_cast<const uint2*>(map)[q];
      l[0] = m.x & 0xFFFFu, l[1] = m.x >> 16, l[2] = m.y & 0xFFFFu, l[3] = m.y >> 16;
    }
    double2* s2 = reinterpret_cast<double2*>(score) + 2 * q;
    double2 x = s2[0], y = s2[1];
    x.x = Blend(x.x, s_lv[l[0]], b);
    x.y = Blend(x.y, s_lv[l[1]], b);
    y.x = Blend(y.x, s_lv[l[2]], b);
    y.y = Blend(y.y, s_lv[l[3]], b);
    s2[0] = x;
    s2[1] = y;
  }
  for (int i = 4 * quads + blockIdx.x * kBAThreads + threadIdx.x; i < n; i += stride) {
    score[i] = Blend(score[i], s_lv[map[i]], b);
  }
}

__global__ __launch_bounds__(256) void k_blend_constant(double* __restrict__ score, int n, double v, ScoreBlend b) {
  const int stride = gridDim.x * blockDim.x;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) score[i] = Blend(score[i], v, b);
}

__global__ __launch_bounds__(256) void k_blend_scale(double* __restrict__ score, int n, double f, bool divide) {
  const int stride = gridDim.x * blockDim.x;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    score[i] = divide ? score[i] / f : score[i] * f;
  }
}

int CappedGrid(int grid, int grid_cap) { return grid_cap > 0 ? std::min(grid, grid_cap) : grid; }

int ElementGrid(int n) { return std::max(1, std::min(DivUp(n, 256), 65536)); }

}  // namespace

void LaunchBlendTraverse(const uint32_t* rowbins, int stride_dw, int width, int n, const CompactTreeDev& t,
                         const ScoreBlend& b, double* score, int num_cu, int grid_cap, hipStream_t s) {
  if (n <= 0) return;
  if (width < 0 || width > 2) Log::Fatal("LaunchBlendTraverse: group-bin width %d", width);
  const size_t lds = ((sizeof(TNode) * t.num_nodes + 15) & ~size_t(15)) + ((sizeof(double) * t.num_leaves + 15) & ~size_t(15)) +
                     (stride_dw <= kTMaxDw ? sizeof(uint32_t) * kTRows * stride_dw : 0);
  const int grid = CappedGrid(TraverseGrid(n, num_cu), grid_cap);
  if (width == 0) {
    k_blend_traverse<0><<<grid, kTThreads, lds, s>>>(rowbins, stride_dw, n, t.nodes, t.num_nodes, t.cats, t.cat_bits,
                                                    t.leaf_value, t.num_leaves, score, b);
  } else if (width == 1) {
    k_blend_traverse<1><<<grid, kTThreads, lds, s>>>(rowbins, stride_dw, n, t.nodes, t.num_nodes, t.cats, t.cat_bits,
                                                    t.leaf_value, t.num_leaves, score, b);
  } else {
    k_blend_traverse<2><<<grid, kTThreads, lds, s>>>(rowbins, stride_dw, n, t.nodes, t.num_nodes, t.cats, t.cat_bits,
                                                    t.leaf_value, t.num_leaves, score, b);
  }
  HIP_CHECK(hipGetLastError());
}

void LaunchBlendTraverseCols(const uint8_t* colbins, int width, int n, const CompactTreeDev& t, const ScoreBlend& b,
                             double* score, int num_cu, int grid_cap, hipStream_t s) {
  if (n <= 0) return;
  if (width != 1 && width != 2) Log::Fatal("LaunchBlendTraverseCols: group-bin width %d (8- / 16-bit rows)", width);
  const size_t lds = ((sizeof(TNode) * t.num_nodes + 15) & ~size_t(15)) + sizeof(double) * t.num_leaves;
  const int grid = CappedGrid(TraverseGrid(n, num_cu), grid_cap);
  if (width == 1) {
    k_blend_traverse_col<1><<<grid, kTThreads, lds, s>>>(colbins, n, t.nodes, t.num_nodes, t.cats, t.cat_bits,
                                                        t.leaf_value, t.num_leaves, score, b);
  } else {
    k_blend_traverse_col<2><<<grid, kTThreads, lds, s>>>(colbins, n, t.nodes, t.num_nodes, t.cats, t.cat_bits,
                                                        t.leaf_value, t.num_leaves, score, b);
  }
  HIP_CHECK(hipGetLastError());
}

void LaunchBlendLeafMapAdd(const void* map, const double* lv, int num_leaves, int n, const ScoreBlend& b,
                           double* score, int num_cu, hipStream_t s) {
  if (n <= 0) return;
  if (num_leaves > kLMMaxLeaves) Log::Fatal("LaunchBlendLeafMapAdd: %d leaves > %d", num_leaves, kLMMaxLeaves);
  // 16-byte score accesses need a 16-byte aligned slice (class k of K starts at k * n rows)
  const bool vec = (reinterpret_cast<uintptr_t>(score) & 15u) == 0;
  const int grid = std::max(1, std::min(DivUp(vec ? DivUp(n, 4) : n, kBAThreads), num_cu * 16));
  if (num_leaves <= 256) {
    k_blend_leaf_add<uint8_t><<<grid, kBAThreads, 0, s>>>(static_cast<const uint8_t*>(map), lv, num_leaves, n, vec, score, b);
  } else {
    k_blend_leaf_add<uint16_t><<<grid, kBAThreads, 0, s>>>(static_cast<const uint16_t*>(map), lv, num_leaves, n, vec, score, b);
  }
  HIP_CHECK(hipGetLastError());
}

void LaunchBlendConstant(double* score, int n, double v, const ScoreBlend& b, hipStream_t s) {
  if (n <= 0) return;
  k_blend_constant<<<ElementGrid(n), 256, 0, s>>>(score, n, v, b);
  HIP_CHECK(hipGetLastError());
}

void LaunchBlendScale(double* score, int n, double f, bool divide, hipStream_t s) {
  if (n <= 0) return;
  k_blend_scale<<<ElementGrid(n), 256, 0, s>>>(score, n, f, divide);
  HIP_CHECK(hipGetLastError());
}

}  // namespace device
}  // namespace lgap
