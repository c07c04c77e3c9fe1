// Prediction from raw feature rows (Booster.predict_device, see predict_kernels.h).
//
// One block takes a tile of rows, staged in LDS with 16-byte loads while the tile fits the LDS
// budget (wider rows are read from global memory: a second instantiation, chosen on the host
// from the shape), and loops over the packed trees in iteration order. Runs of consecutive
// trees are staged cooperatively into LDS (nodes and leaf values); a tree larger than the tree
// budget is walked from global memory. Every lane walks kPRowsPerThread rows, interleaved level
// by level so their node and feature reads overlap, and adds each tree's output to its rows'
// fp64 accumulators in tree order: the host's out[k] += Predict(x) order, so raw scores are
// bit-identical. No atomics, no cross-lane reduction. The walk itself is predict_pack.h's.
//
// ResidentEnsemble keeps the packed ensemble, the batch plan, a stream and grow-only buffers on
// the device for repeated calls (Booster.device_predictor); PredictDense is a temporary one. For
// batches of at most tree_parallel_rows rows it launches k_predict_pairs (one work item per row
// and tree, into a [tree][row] scratch) and k_predict_fold (one lane per row and class, adding
// in the same order), so that a handful of rows is spread over the chip.
#include "device/predict_kernels.h"

#include <algorithm>

#include "device/hip_common.h"
#include "lgap/device_api.h"
#include "lgap/log.h"
#include "lgap/pointwise_metric.h"

namespace lgap {
namespace device {

std::vector<PredictBatch> PlanPredictBatches(const PackedEnsemble& pk) {
  std::vector<PredictBatch> out;
  const int n = static_cast<int>(pk.trees.size());
  int i = 0;
  while (i < n) {
    PredictBatch b{};
    b.first = i;
    b.node_begin = pk.trees[i].node_off;
    b.leaf_begin = pk.trees[i].leaf_off;
    int nodes = 0, leaves = 0, j = i;
    while (j < n) {
      const int L = pk.trees[j].num_leaves;
      if (PredictTreeLdsBytes(nodes + L - 1, leaves + L) > static_cast<size_t>(kPTreeLdsBytes)) break;
      nodes += L - 1;
      leaves += L;
      ++j;
    }
    if (j == i) {  // this tree alone exceeds the budget: walked from global memory
      b.count = 1;
      b.node_count = pk.trees[i].num_leaves - 1;
      b.leaf_count = pk.trees[i].num_leaves;
      b.staged = 0;
      i += 1;
    } else {
      b.count = j - i;
      b.node_count = nodes;
      b.leaf_count = leaves;
      b.staged = 1;
      i = j;
    }
    out.push_back(b);
  }
  return out;
}

PredictShape PlanPredictShape(int ncol, size_t elem, int num_tree_per_iteration, bool leaf) {
  PredictShape s{};
  s.tile_rows = kPTileRows;
  s.acc_lds = (!leaf && num_tree_per_iteration > kPRegClasses) ? 1 : 0;
  size_t acc_bytes = 0;
  if (s.acc_lds) {
    const size_t per_row = sizeof(double) * static_cast<size_t>(num_tree_per_iteration);
    if (per_row > static_cast<size_t>(kPTileLdsBytes)) {
      Log::Fatal("predict_device: %d trees per iteration exceed the accumulator budget (%d); use Booster.predict",
                 num_tree_per_iteration, kPTileLdsBytes / static_cast<int>(sizeof(double)));
    }
    int rows = static_cast<int>(std::min<size_t>(kPTileRows, kPTileLdsBytes / per_row));
    if (rows >= 64) rows &= ~63;
    s.tile_rows = rows;
    acc_bytes = (per_row * rows + 15) & ~static_cast<size_t>(15);
  }
  const size_t row_bytes = static_cast<size_t>(s.tile_rows) * ncol * elem;
  s.stage_rows = acc_bytes + row_bytes <= static_cast<size_t>(kPTileLdsBytes) ? 1 : 0;
  s.lds_bytes = kPTreeLdsBytes + acc_bytes + (s.stage_rows ? ((row_bytes + 15) & ~static_cast<size_t>(15)) : 0);
  return s;
}

PairShape PlanPairShape(int nrow, int ncol, size_t elem, int num_batches) {
  PairShape s{};
  s.tile_rows = nrow <= kPairSmallTileMaxRows ? kPairSmallTileRows : kPairLargeTileRows;
  const size_t row_bytes = static_cast<size_t>(s.tile_rows) * ncol * elem;
  s.stage_rows = row_bytes <= static_cast<size_t>(kPairRowLdsBytes) ? 1 : 0;
  s.lds_bytes = kPTreeLdsBytes + (s.stage_rows ? ((row_bytes + 15) & ~static_cast<size_t>(15)) : 0);
  const long long tiles = (static_cast<long long>(nrow) + s.tile_rows - 1) / s.tile_rows;
  s.grid = tiles * num_batches;
  return s;
}

namespace {

struct PredictArgs {
  PackedView v;  // device pointers
  const PredictBatch* batches;
  int num_batches;
  const void* rows;
  long long n;
  int ncol;
  int tile_rows;
  double* out;
};

constexpr int kR = kPRowsPerThread;

// One tree over the lane's rows. KR: accumulators per row in registers (0: in LDS, s_acc[k][row]).
template <typename T, int KR, bool LEAF>
__device__ __forceinline__ void WalkTree(const PredictArgs& a, const PTree& tr, int tree, int k, const PNode* nodes,
                                         const double* leaves, const T* const (&row)[kR], const bool (&act)[kR],
                                         double (&acc)[kR][KR > 0 ? KR : 1], double* s_acc, long long base) {
  int node[kR];
#pragma unroll
  for (int j = 0; j < kR; ++j) node[j] = ~0;  // a one-leaf tree: leaf 0
  if (tr.num_leaves > 1) {
    const int32_t* cat_b = a.v.cat_boundaries + tr.cat_off;
#pragma unroll
    for (int j = 0; j < kR; ++j) node[j] = act[j] ? 0 : ~0;
    // one level of all walks per pass: the node reads, then the feature reads issued together
    // (finished walks re-read the root and drop the result), then the decisions
    bool live = true;
    while (live) {
      live = false;
      PNode nd[kR];
      double fv[kR];
#pragma unroll
      for (int j = 0; j < kR; ++j) nd[j] = nodes[node[j] < 0 ? 0 : node[j]];
#pragma unroll
      for (int j = 0; j < kR; ++j) fv[j] = PredFeature(row[j], a.ncol, nd[j].split_feature);
#pragma unroll
      for (int j = 0; j < kR; ++j) {
        if (node[j] < 0) continue;
        node[j] = PredDecide(nd[j], fv[j], cat_b, a.v.cat_threshold);
        live |= node[j] >= 0;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < kR; ++j) {
    if (!act[j]) continue;
    const int r = static_cast<int>(threadIdx.x) + j * kPThreads;
    const int leaf = ~node[j];
    if (LEAF) {
      a.out[static_cast<size_t>(base + r) * a.v.num_trees + tree] = static_cast<double>(leaf);
    } else {
      const double val = PredLeafOutput(a.v, tr, leaf, leaves[leaf], row[j], a.ncol);
      if (KR == 0) {
        s_acc[static_cast<size_t>(k) * a.tile_rows + r] += val;
      } else {
#pragma unroll
        for (int c = 0; c < (KR > 0 ? KR : 1); ++c) {
          const double sum = acc[j][c] + val;
          acc[j][c] = c == k ? sum : acc[j][c];  // a select per register, never an indexed store
        }
      }
    }
  }
}

template <typename T, int KR, bool LEAF, bool STAGE>
__device__ __forceinline__ void PredictBody(const PredictArgs& a) {
  extern __shared__ __align__(16) unsigned char lds[];
  const int K = a.v.num_tree_per_iteration;
  const int tile = a.tile_rows;
  PNode* s_nodes = reinterpret_cast<PNode*>(lds);
  double* s_acc = reinterpret_cast<double*>(lds + kPTreeLdsBytes);
  const size_t acc_bytes =
      (!LEAF && KR == 0) ? ((sizeof(double) * static_cast<size_t>(K) * tile + 15) & ~static_cast<size_t>(15)) : 0;
  T* s_rows = reinterpret_cast<T*>(lds + kPTreeLdsBytes + acc_bytes);
  const T* g_rows = static_cast<const T*>(a.rows);
  const int t = threadIdx.x;
  for (long long base = static_cast<long long>(blockIdx.x) * tile; base < a.n;
       base += static_cast<long long>(gridDim.x) * tile) {
    const int rows = static_cast<int>(min(static_cast<long long>(tile), a.n - base));
    if (STAGE) {
      __syncthreads();  // the previous tile's walks are done
      const T* src = g_rows + base * a.ncol;
      const int nel = rows * a.ncol;
      constexpr int kPer16 = 16 / static_cast<int>(sizeof(T));
      const int nq = (reinterpret_cast<uintptr_t>(src) & 15u) == 0 ? nel / kPer16 : 0;
      const uint4* src4 = reinterpret_cast<const uint4*>(src);
      uint4* dst4 = reinterpret_cast<uint4*>(s_rows);
      for (int q = t; q < nq; q += kPThreads) dst4[q] = src4[q];
      for (int q = nq * kPer16 + t; q < nel; q += kPThreads) s_rows[q] = src[q];
      // visible to every lane after the first barrier of the batch loop
    }
    const T* row[kR];
    bool act[kR];
    double acc[kR][KR > 0 ? KR : 1];
#pragma unroll
    for (int j = 0; j < kR; ++j) {
      const int r = t + j * kPThreads;
      act[j] = r < rows;
      const int rr = act[j] ? r : 0;  // idle walks read the tile's first row
      row[j] = STAGE ? s_rows + static_cast<size_t>(rr) * a.ncol : g_rows + static_cast<size_t>(base + rr) * a.ncol;
#pragma unroll
      for (int c = 0; c < (KR > 0 ? KR : 1); ++c) acc[j][c] = 0.0;
      if (!LEAF && KR == 0 && act[j]) {
        for (int c = 0; c < K; ++c) s_acc[static_cast<size_t>(c) * tile + r] = 0.0;  // this lane's own slots
      }
    }
    for (int b = 0; b < a.num_batches; ++b) {
      const PredictBatch bt = a.batches[b];
      double* s_leaf = reinterpret_cast<double*>(
          lds + ((sizeof(PNode) * static_cast<size_t>(bt.node_count) + 15) & ~static_cast<size_t>(15)));
      __syncthreads();  // the previous batch's walks are done (first batch: the staged rows are in place)
      if (bt.staged) {
        const uint32_t* nsrc = reinterpret_cast<const uint32_t*>(a.v.nodes + bt.node_begin);
        const int ndw = bt.node_count * static_cast<int>(sizeof(PNode) / 4);
        for (int q = t; q < ndw; q += kPThreads) reinterpret_cast<uint32_t*>(s_nodes)[q] = nsrc[q];
        const double* lsrc = a.v.leaf_value + bt.leaf_begin;
        for (int q = t; q < bt.leaf_count; q += kPThreads) s_leaf[q] = lsrc[q];
        __syncthreads();
      }
      for (int ti = 0; ti < bt.count; ++ti) {
        const int tree = bt.first + ti;
        const PTree tr = a.v.trees[tree];
        const int k = tree % K;
        if (bt.staged) {
          WalkTree<T, KR, LEAF>(a, tr, tree, k, s_nodes + (tr.node_off - bt.node_begin),
                                s_leaf + (tr.leaf_off - bt.leaf_begin), row, act, acc, s_acc, base);
        } else {
          WalkTree<T, KR, LEAF>(a, tr, tree, k, a.v.nodes + tr.node_off, a.v.leaf_value + tr.leaf_off, row, act, acc,
                                s_acc, base);
        }
      }
    }
    if (!LEAF) {
      // GBDT::PredictRaw: average_output divides by the iteration count at the end
      const bool avg = a.v.average_output && a.v.num_iterations > 0;
#pragma unroll
      for (int j = 0; j < kR; ++j) {
        if (!act[j]) continue;
        const int r = t + j * kPThreads;
        double* o = a.out + static_cast<size_t>(base + r) * K;
        if (KR == 0) {
          for (int c = 0; c < K; ++c) {
            double v = s_acc[static_cast<size_t>(c) * tile + r];
            if (avg) v /= a.v.num_iterations;
            o[c] = v;
          }
        } else {
#pragma unroll
          for (int c = 0; c < (KR > 0 ? KR : 1); ++c) {
            if (c < K) {
              double v = acc[j][c];
              if (avg) v /= a.v.num_iterations;
              o[c] = v;
            }
          }
        }
      }
    }
  }
}

template <typename T, int KR, bool STAGE>
__global__ __launch_bounds__(kPThreads) void k_predict_raw(PredictArgs a) {
  PredictBody<T, KR, false, STAGE>(a);
}

template <typename T, bool STAGE>
__global__ __launch_bounds__(kPThreads) void k_predict_leaf(PredictArgs a) {
  PredictBody<T, 1, true, STAGE>(a);
}

// The objective's output transform on device-resident raw scores, in place: s[row][K].
__global__ __launch_bounds__(kPThreads) void k_predict_convert(double* __restrict__ s, long long n, int K,
                                                               PredictTransform tf) {
  PwMetricParams p;
  p.output = tf.output;
  p.sigmoid = tf.sigmoid;
  for (long long i = static_cast<long long>(blockIdx.x) * kPThreads + threadIdx.x; i < n;
       i += static_cast<long long>(gridDim.x) * kPThreads) {
    double* o = s + i * K;
    if (tf.kind == kTransformSoftmax) {  // common::Softmax
      double wmax = o[0];
      for (int k = 1; k < K; ++k) wmax = fmax(wmax, o[k]);
      double sum = 0.0;
      for (int k = 0; k < K; ++k) {
        o[k] = exp(o[k] - wmax);
        sum += o[k];
      }
      for (int k = 0; k < K; ++k) o[k] /= sum;
    } else if (tf.kind == kTransformOVA) {
      for (int k = 0; k < K; ++k) o[k] = 1.0f / (1.0f + exp(-tf.sigmoid * o[k]));
    } else if (tf.kind == kTransformPointwise) {
      for (int k = 0; k < K; ++k) o[k] = PmConvert(p, o[k]);
    }
  }
}

// ---- the tree-parallel path: one work item per (row, tree) pair, then a fold per (row, class).
// A 1-row batch still gets one lane per tree of a run and one block per run, where the
// row-parallel kernel gives the whole forest to one lane.
struct PairArgs {
  PackedView v;  // device pointers
  const PredictBatch* batches;
  int num_batches;
  const void* rows;
  int n;          // rows of this launch, the stride of vals
  int ncol;
  int tile_rows;
  double* vals;   // raw: [tree][n]
  double* out;    // leaf: [n][num_trees], final
};

// Block (tile, batch) = (blockIdx.x / num_batches, blockIdx.x % num_batches): neighbouring
// blocks read the same rows. Pair p of the block is row p % rows of tree p / rows, so a wave
// writes consecutive rows of one tree. Exactly one lane writes each element.
template <typename T, bool LEAF, bool STAGE>
__global__ __launch_bounds__(kPThreads) void k_predict_pairs(PairArgs a) {
  extern __shared__ __align__(16) unsigned char lds[];
  const int t = threadIdx.x;
  const int tile = static_cast<int>(blockIdx.x / static_cast<unsigned>(a.num_batches));
  const PredictBatch bt = a.batches[blockIdx.x - static_cast<unsigned>(tile) * a.num_batches];
  const int base = tile * a.tile_rows;
  const int rows = min(a.tile_rows, a.n - base);
  PNode* s_nodes = reinterpret_cast<PNode*>(lds);
  double* s_leaf = reinterpret_cast<double*>(
      lds + ((sizeof(PNode) * static_cast<size_t>(bt.node_count) + 15) & ~static_cast<size_t>(15)));
  T* s_rows = reinterpret_cast<T*>(lds + kPTreeLdsBytes);
  const T* g_rows = static_cast<const T*>(a.rows) + static_cast<size_t>(base) * a.ncol;
  if (bt.staged) {
    const uint32_t* nsrc = reinterpret_cast<const uint32_t*>(a.v.nodes + bt.node_begin);
    const int ndw = bt.node_count * static_cast<int>(sizeof(PNode) / 4);
    for (int q = t; q < ndw; q += kPThreads) reinterpret_cast<uint32_t*>(s_nodes)[q] = nsrc[q];
    const double* lsrc = a.v.leaf_value + bt.leaf_begin;
    for (int q = t; q < bt.leaf_count; q += kPThreads) s_leaf[q] = lsrc[q];
  }
  if (STAGE) {
    const int nel = rows * a.ncol;
    constexpr int kPer16 = 16 / static_cast<int>(sizeof(T));
    const int nq = (reinterpret_cast<uintptr_t>(g_rows) & 15u) == 0 ? nel / kPer16 : 0;
    const uint4* src4 = reinterpret_cast<const uint4*>(g_rows);
    uint4* dst4 = reinterpret_cast<uint4*>(s_rows);
    for (int q = t; q < nq; q += kPThreads) dst4[q] = src4[q];
    for (int q = nq * kPer16 + t; q < nel; q += kPThreads) s_rows[q] = g_rows[q];
  }
  __syncthreads();
  const int pairs = rows * bt.count;
  for (int p = t; p < pairs; p += kPThreads) {
    const int ti = p / rows;
    const int r = p - ti * rows;
    const int tree = bt.first + ti;
    const PTree tr = a.v.trees[tree];
    const PNode* nodes = bt.staged ? s_nodes + (tr.node_off - bt.node_begin) : a.v.nodes + tr.node_off;
    const double* leaves = bt.staged ? s_leaf + (tr.leaf_off - bt.leaf_begin) : a.v.leaf_value + tr.leaf_off;
    const T* row = (STAGE ? s_rows : g_rows) + static_cast<size_t>(r) * a.ncol;
    if (LEAF) {
      const int leaf = PredLeaf(nodes, tr.num_leaves, a.v.cat_boundaries + tr.cat_off, a.v.cat_threshold, row, a.ncol);
      a.out[static_cast<size_t>(base + r) * a.v.num_trees + tree] = static_cast<double>(leaf);
    } else {
      a.vals[static_cast<size_t>(tree) * a.n + (base + r)] = PredPairValue(a.v, tr, nodes, leaves, row, a.ncol);
    }
  }
}

// One lane per (row, class): lane i is row i % n of class i / n, so a wave reads consecutive
// rows of each tree. The sum itself is predict_pack.h's.
__global__ __launch_bounds__(kPThreads) void k_predict_fold(PackedView v, const double* __restrict__ vals, int n,
                                                            double* __restrict__ out) {
  const int K = v.num_tree_per_iteration;
  const long long total = static_cast<long long>(n) * K;
  for (long long i = static_cast<long long>(blockIdx.x) * kPThreads + threadIdx.x; i < total;
       i += static_cast<long long>(gridDim.x) * kPThreads) {
    const int k = static_cast<int>(i / n);
    const long long row = i - static_cast<long long>(k) * n;
    out[row * K + k] = PredFoldRow(v, vals, n, row, k);
  }
}

template <typename T>
void LaunchPairs(const PairArgs& a, bool leaf, const PairShape& sh, hipStream_t s) {
  const unsigned grid = static_cast<unsigned>(sh.grid);
  const size_t lds = sh.lds_bytes;
  if (leaf) {
    if (sh.stage_rows) k_predict_pairs<T, true, true><<<grid, kPThreads, lds, s>>>(a);
    else k_predict_pairs<T, true, false><<<grid, kPThreads, lds, s>>>(a);
  } else {
    if (sh.stage_rows) k_predict_pairs<T, false, true><<<grid, kPThreads, lds, s>>>(a);
    else k_predict_pairs<T, false, false><<<grid, kPThreads, lds, s>>>(a);
  }
  HIP_CHECK(hipGetLastError());
}

template <typename T>
void LaunchPredict(const PredictArgs& a, int mode, const PredictShape& sh, int num_cu, hipStream_t s) {
  const long long tiles = (a.n + sh.tile_rows - 1) / sh.tile_rows;
  // blocks per CU by LDS (160 KiB per CU), at most 8
  const int per_cu = static_cast<int>(std::max<size_t>(1, std::min<size_t>(8, (size_t(160) << 10) / sh.lds_bytes)));
  const int grid = static_cast<int>(std::max<long long>(1, std::min<long long>(tiles, static_cast<long long>(num_cu) * per_cu)));
  const size_t lds = sh.lds_bytes;
  const int K = a.v.num_tree_per_iteration;
  if (mode == kPredictLeaf) {
    if (sh.stage_rows) k_predict_leaf<T, true><<<grid, kPThreads, lds, s>>>(a);
    else k_predict_leaf<T, false><<<grid, kPThreads, lds, s>>>(a);
  } else if (K == 1) {
    if (sh.stage_rows) k_predict_raw<T, 1, true><<<grid, kPThreads, lds, s>>>(a);
    else k_predict_raw<T, 1, false><<<grid, kPThreads, lds, s>>>(a);
  } else if (!sh.acc_lds) {
    if (sh.stage_rows) k_predict_raw<T, kPRegClasses, true><<<grid, kPThreads, lds, s>>>(a);
    else k_predict_raw<T, kPRegClasses, false><<<grid, kPThreads, lds, s>>>(a);
  } else {
    if (sh.stage_rows) k_predict_raw<T, 0, true><<<grid, kPThreads, lds, s>>>(a);
    else k_predict_raw<T, 0, false><<<grid, kPThreads, lds, s>>>(a);
  }
  HIP_CHECK(hipGetLastError());
}

struct ScopedStream {
  hipStream_t s = nullptr;
  ScopedStream() { HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
  ~ScopedStream() {
    if (s) (void)hipStreamDestroy(s);
  }
};

template <typename T>
void UploadOrOne(DevBuf<T>* buf, const std::vector<T>& v, hipStream_t s) {
  if (v.empty()) buf->Resize(1);  // never a null array in the view
  else buf->Upload(v, s);
}

}  // namespace

// ---- the resident ensemble: everything a call needs, uploaded or allocated once
struct ResidentEnsemble::Impl {
  ScopedStream st;
  int dev = 0, num_cu = 256;
  int tree_parallel_rows = 0;
  bool pinned = false;
  PackedView v;  // device pointers
  DevBuf<PNode> d_nodes;
  DevBuf<PTree> d_trees;
  DevBuf<int32_t> d_catb, d_linoff, d_linfeat;
  DevBuf<uint32_t> d_catt;
  DevBuf<double> d_leaf, d_linconst, d_lincoef;
  DevBuf<PredictBatch> d_batches;
  int num_batches = 0;
  // grow-only work buffers
  DevBuf<char> d_in;
  DevBuf<double> d_out, d_vals;
  PinnedBuf<char> h_in;
  PinnedBuf<double> h_out;

  template <typename T>
  static void Grow(DevBuf<T>* buf, size_t n) {
    if (n > buf->size()) buf->Resize(n);
  }
};

ResidentEnsemble::ResidentEnsemble(const PackedEnsemble& pk, int tree_parallel_rows, bool pinned) {
  if (DeviceCount() <= 0) {
    Log::Fatal("predict_device: no gfx950 GPU is visible to this process; use Booster.predict for host prediction");
  }
  if (tree_parallel_rows < 0 || tree_parallel_rows > kTreeParallelMaxRows) {
    Log::Fatal("device_predictor: tree_parallel_rows must be between 0 and %d, got %d", kTreeParallelMaxRows,
               tree_parallel_rows);
  }
  impl_ = std::make_unique<Impl>();
  Impl& m = *impl_;
  m.tree_parallel_rows = tree_parallel_rows;
  m.pinned = pinned;
  hipStream_t s = m.st.s;
  HIP_CHECK(hipGetDevice(&m.dev));
  HIP_CHECK(hipDeviceGetAttribute(&m.num_cu, hipDeviceAttributeMultiprocessorCount, m.dev));
  const std::vector<PredictBatch> batches = PlanPredictBatches(pk);
  m.num_batches = static_cast<int>(batches.size());
  UploadOrOne(&m.d_nodes, pk.nodes, s);
  UploadOrOne(&m.d_trees, pk.trees, s);
  UploadOrOne(&m.d_catb, pk.cat_boundaries, s);
  UploadOrOne(&m.d_catt, pk.cat_threshold, s);
  UploadOrOne(&m.d_leaf, pk.leaf_value, s);
  UploadOrOne(&m.d_linconst, pk.lin_const, s);
  UploadOrOne(&m.d_linoff, pk.lin_off, s);
  UploadOrOne(&m.d_lincoef, pk.lin_coef, s);
  UploadOrOne(&m.d_linfeat, pk.lin_feat, s);
  UploadOrOne(&m.d_batches, batches, s);
  m.v = pk.View();
  m.v.nodes = m.d_nodes.get();
  m.v.trees = m.d_trees.get();
  m.v.cat_boundaries = m.d_catb.get();
  m.v.cat_threshold = m.d_catt.get();
  m.v.leaf_value = m.d_leaf.get();
  m.v.lin_const = m.d_linconst.get();
  m.v.lin_off = m.d_linoff.get();
  m.v.lin_coef = m.d_lincoef.get();
  m.v.lin_feat = m.d_linfeat.get();
  // `pk` and `batches` may go away when this returns: the uploads read them until the stream is idle
  HIP_CHECK(hipStreamSynchronize(s));
}

ResidentEnsemble::~ResidentEnsemble() = default;

void ResidentEnsemble::Predict(const void* data, bool f64, int nrow, int ncol, int mode,
                               const PredictTransform* transform, bool data_on_device, bool out_on_device,
                               double* out) {
  Impl& m = *impl_;
  if (nrow <= 0) return;
  if (ncol <= 0) Log::Fatal("predict_device: the data has no columns");
  const bool leaf = mode == kPredictLeaf;
  const int width = PredictWidth(m.v, mode);
  if (width <= 0) return;
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  if (dev != m.dev) {
    Log::Fatal("device_predictor: created on device %d and called with device %d current", m.dev, dev);
  }
  hipStream_t s = m.st.s;
  const size_t es = f64 ? 8 : 4;
  const int K = m.v.num_tree_per_iteration;
  const bool tree_path = nrow <= m.tree_parallel_rows;

  // Rows in chunks of at most 256 MiB of input (and of output, which is wider for leaf indices,
  // and of the tree-parallel scratch); device-resident input and output are used in place,
  // chunk by chunk.
  const size_t row_bytes = es * static_cast<size_t>(ncol);
  const size_t out_row_bytes = sizeof(double) * static_cast<size_t>(width);
  const size_t cap = size_t(256) << 20;
  size_t chunk = nrow;
  if (!data_on_device) chunk = std::min(chunk, std::max<size_t>(1, cap / row_bytes));
  if (!out_on_device) chunk = std::min(chunk, std::max<size_t>(1, cap / out_row_bytes));
  if (tree_path && !leaf && m.v.num_trees > 0) {
    chunk = std::min(chunk, std::max<size_t>(1, cap / (sizeof(double) * static_cast<size_t>(m.v.num_trees))));
  }
  if (!data_on_device) Impl::Grow(&m.d_in, row_bytes * chunk);
  if (!out_on_device) Impl::Grow(&m.d_out, static_cast<size_t>(width) * chunk);
  if (tree_path && !leaf) Impl::Grow(&m.d_vals, std::max<size_t>(1, static_cast<size_t>(m.v.num_trees) * chunk));
  char* h_in = (m.pinned && !data_on_device) ? m.h_in.Get(row_bytes * chunk) : nullptr;
  double* h_out = (m.pinned && !out_on_device) ? m.h_out.Get(static_cast<size_t>(width) * chunk) : nullptr;

  PredictShape sh{};
  PredictArgs a{};
  if (!tree_path) {
    sh = PlanPredictShape(ncol, es, K, leaf);
    a.v = m.v;
    a.batches = m.d_batches.get();
    a.num_batches = m.num_batches;
    a.ncol = ncol;
    a.tile_rows = sh.tile_rows;
  }
  for (size_t r0 = 0; r0 < static_cast<size_t>(nrow); r0 += chunk) {
    const size_t rows = std::min(chunk, static_cast<size_t>(nrow) - r0);
    const char* src = static_cast<const char*>(data) + row_bytes * r0;
    const void* d_rows = src;
    if (!data_on_device) {
      if (h_in != nullptr) {
        if (r0 > 0) HIP_CHECK(hipStreamSynchronize(s));  // the previous chunk's upload has left the buffer
        CopyHostBytes(h_in, src, row_bytes * rows);
        src = h_in;
      }
      HIP_CHECK(hipMemcpyAsync(m.d_in.get(), src, row_bytes * rows, hipMemcpyHostToDevice, s));
      d_rows = m.d_in.get();
    }
    double* d_res = out_on_device ? out + r0 * width : m.d_out.get();
    if (tree_path) {
      const PairShape ps = PlanPairShape(static_cast<int>(rows), ncol, es, m.num_batches);
      if (ps.grid > static_cast<long long>(INT32_MAX)) {
        Log::Fatal("device_predictor: %lld blocks exceed the grid of the tree-parallel kernel; lower tree_parallel_rows",
                   ps.grid);
      }
      PairArgs pa{};
      pa.v = m.v;
      pa.batches = m.d_batches.get();
      pa.num_batches = m.num_batches;
      pa.rows = d_rows;
      pa.n = static_cast<int>(rows);
      pa.ncol = ncol;
      pa.tile_rows = ps.tile_rows;
      pa.vals = m.d_vals.get();
      pa.out = d_res;
      if (ps.grid > 0) {
        if (f64) LaunchPairs<double>(pa, leaf, ps, s);
        else LaunchPairs<float>(pa, leaf, ps, s);
      }
      if (!leaf) {
        const long long lanes = static_cast<long long>(rows) * K;
        const int grid = static_cast<int>(std::max<long long>(
            1, std::min<long long>((lanes + kPThreads - 1) / kPThreads, static_cast<long long>(m.num_cu) * 8)));
        k_predict_fold<<<grid, kPThreads, 0, s>>>(m.v, m.d_vals.get(), static_cast<int>(rows), d_res);
        HIP_CHECK(hipGetLastError());
      }
    } else {
      a.rows = d_rows;
      a.out = d_res;
      a.n = static_cast<long long>(rows);
      if (f64) LaunchPredict<double>(a, mode, sh, m.num_cu, s);
      else LaunchPredict<float>(a, mode, sh, m.num_cu, s);
    }
    if (!leaf && transform != nullptr && transform->kind != kTransformIdentity && out_on_device) {
      const long long n = static_cast<long long>(rows);
      const int grid = static_cast<int>(std::max<long long>(
          1, std::min<long long>((n + kPThreads - 1) / kPThreads, static_cast<long long>(m.num_cu) * 8)));
      k_predict_convert<<<grid, kPThreads, 0, s>>>(d_res, n, width, *transform);
      HIP_CHECK(hipGetLastError());
    }
    if (!out_on_device) {
      double* dst = h_out != nullptr ? h_out : out + r0 * width;
      HIP_CHECK(hipMemcpyAsync(dst, m.d_out.get(), out_row_bytes * rows, hipMemcpyDeviceToHost, s));
      if (h_out != nullptr) {  // the staging buffer is reused by the next chunk
        HIP_CHECK(hipStreamSynchronize(s));
        CopyHostBytes(out + r0 * width, h_out, out_row_bytes * rows);
      }
    }
  }
  HIP_CHECK(hipStreamSynchronize(s));
  last_path_ = tree_path ? kPathTree : kPathRow;
}

// One launch path: a temporary resident ensemble, row-parallel kernels, the caller's memory
// copied as it is (pinning staging buffers for a single call costs more than it saves).
void PredictDense(const PackedEnsemble& pk, const void* data, bool f64, int nrow, int ncol, int mode,
                  const PredictTransform* transform, bool data_on_device, bool out_on_device, double* out) {
  if (DeviceCount() <= 0) {
    Log::Fatal("predict_device: no gfx950 GPU is visible to this process; use Booster.predict for host prediction");
  }
  if (nrow <= 0) return;
  if (ncol <= 0) Log::Fatal("predict_device: the data has no columns");
  if (PredictWidth(pk.View(), mode) <= 0) return;
  ResidentEnsemble re(pk, 0, false);
  re.Predict(data, f64, nrow, ncol, mode, transform, data_on_device, out_on_device, out);
}

}  // namespace device
}  // namespace lgap
