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

void PredictDense(const PackedEnsemble& pk, const void* data, bool f64, int nrow, int ncol, int mode,
                  const PredictTransform* transform, bool data_on_device, bool out_on_device, double* out) {
  if (DeviceCount() <= 0) {
    Log::Fatal("predict_device: no gfx950 GPU is visible to this process; use Booster.predict for host prediction");
  }
  if (nrow <= 0) return;
  if (ncol <= 0) Log::Fatal("predict_device: the data has no columns");
  const bool leaf = mode == kPredictLeaf;
  PackedView hv = pk.View();
  const int width = PredictWidth(hv, mode);
  if (width <= 0) return;
  const size_t es = f64 ? 8 : 4;
  const PredictShape sh = PlanPredictShape(ncol, es, pk.num_tree_per_iteration, leaf);
  const std::vector<PredictBatch> batches = PlanPredictBatches(pk);

  ScopedStream st;
  hipStream_t s = st.s;
  int dev = 0, num_cu = 256;
  HIP_CHECK(hipGetDevice(&dev));
  HIP_CHECK(hipDeviceGetAttribute(&num_cu, hipDeviceAttributeMultiprocessorCount, dev));

  DevBuf<PNode> d_nodes;
  DevBuf<PTree> d_trees;
  DevBuf<int32_t> d_catb, d_linoff, d_linfeat;
  DevBuf<uint32_t> d_catt;
  DevBuf<double> d_leaf, d_linconst, d_lincoef;
  DevBuf<PredictBatch> d_batches;
  UploadOrOne(&d_nodes, pk.nodes, s);
  UploadOrOne(&d_trees, pk.trees, s);
  UploadOrOne(&d_catb, pk.cat_boundaries, s);
  UploadOrOne(&d_catt, pk.cat_threshold, s);
  UploadOrOne(&d_leaf, pk.leaf_value, s);
  UploadOrOne(&d_linconst, pk.lin_const, s);
  UploadOrOne(&d_linoff, pk.lin_off, s);
  UploadOrOne(&d_lincoef, pk.lin_coef, s);
  UploadOrOne(&d_linfeat, pk.lin_feat, s);
  UploadOrOne(&d_batches, batches, s);

  PredictArgs a{};
  a.v = hv;
  a.v.nodes = d_nodes.get();
  a.v.trees = d_trees.get();
  a.v.cat_boundaries = d_catb.get();
  a.v.cat_threshold = d_catt.get();
  a.v.leaf_value = d_leaf.get();
  a.v.lin_const = d_linconst.get();
  a.v.lin_off = d_linoff.get();
  a.v.lin_coef = d_lincoef.get();
  a.v.lin_feat = d_linfeat.get();
  a.batches = d_batches.get();
  a.num_batches = static_cast<int>(batches.size());
  a.ncol = ncol;
  a.tile_rows = sh.tile_rows;

  // Rows in chunks of at most 256 MiB of input (and of output, which is wider for leaf
  // indices); device-resident input and output are used in place, chunk by chunk.
  const size_t row_bytes = es * static_cast<size_t>(ncol);
  const size_t out_row_bytes = sizeof(double) * static_cast<size_t>(width);
  const size_t cap = size_t(256) << 20;
  size_t chunk = nrow;
  if (!data_on_device) chunk = std::min(chunk, std::max<size_t>(1, cap / row_bytes));
  if (!out_on_device) chunk = std::min(chunk, std::max<size_t>(1, cap / out_row_bytes));
  DevBuf<char> d_in;
  DevBuf<double> d_out;
  if (!data_on_device) d_in.Resize(row_bytes * chunk);
  if (!out_on_device) d_out.Resize(static_cast<size_t>(width) * chunk);
  for (size_t r0 = 0; r0 < static_cast<size_t>(nrow); r0 += chunk) {
    const size_t rows = std::min(chunk, static_cast<size_t>(nrow) - r0);
    const char* src = static_cast<const char*>(data) + row_bytes * r0;
    if (!data_on_device) {
      HIP_CHECK(hipMemcpyAsync(d_in.get(), src, row_bytes * rows, hipMemcpyHostToDevice, s));
      a.rows = d_in.get();
    } else {
      a.rows = src;
    }
    a.out = out_on_device ? out + r0 * width : d_out.get();
    a.n = static_cast<long long>(rows);
    if (f64) LaunchPredict<double>(a, mode, sh, num_cu, s);
    else LaunchPredict<float>(a, mode, sh, num_cu, s);
    if (!leaf && transform != nullptr && transform->kind != kTransformIdentity && out_on_device) {
      const int grid = static_cast<int>(std::max<long long>(
          1, std::min<long long>((a.n + kPThreads - 1) / kPThreads, static_cast<long long>(num_cu) * 8)));
      k_predict_convert<<<grid, kPThreads, 0, s>>>(a.out, a.n, width, *transform);
      HIP_CHECK(hipGetLastError());
    }
    if (!out_on_device) {
      HIP_CHECK(hipMemcpyAsync(out + r0 * width, d_out.get(), out_row_bytes * rows, hipMemcpyDeviceToHost, s));
    }
  }
  HIP_CHECK(hipStreamSynchronize(s));
}

}  // namespace device
}  // namespace lgap
