// SHAP values from raw feature rows (Booster.predict_contrib_device, see contrib_kernels.h).
//
// One lane owns one row; a block takes a tile of blockDim.x rows and walks the whole selected
// ensemble for it with contrib_pack.h's ContribRow, the function the host hook runs. All lanes
// of a wave are on the same path at the same time: path metadata (features, z, edges, nodes,
// leaf value) is wave-uniform, only the row's feature values and one fractions differ. The
// lane's weight array lives in LDS as [slot][lane] (conflict-free), its contribution row in
// LDS as [column][lane] while the tile fits (written out coalesced at the end) and otherwise
// in its own output row in global memory; rows are staged in LDS with 16-byte loads when they
// fit. Every output element is produced by one lane in a fixed order: no atomics, no cross-lane
// reduction, the same bits as the host hook. Row tiles are the only parallelism: a batch of
// fewer rows than the GPU has lanes leaves part of it idle.
#include "device/contrib_kernels.h"

#include <algorithm>

#include "device/hip_common.h"
#include "lgap/device_api.h"
#include "lgap/log.h"

namespace lgap {
namespace device {

namespace {

struct ContribArgs {
  ContribView v;  // device pointers
  const void* rows;
  long long n;
  int ncol;
  int w_slots;
  int width;
  double* out;
};

template <typename T, bool STAGE, bool PHI_LDS>
__global__ __launch_bounds__(kCMaxThreads) void k_predict_contrib(ContribArgs a) {
  extern __shared__ __align__(16) unsigned char lds[];
  const int threads = blockDim.x;
  const int t = threadIdx.x;
  const int width = a.width;
  double* s_w = reinterpret_cast<double*>(lds);
  double* s_phi = s_w + static_cast<size_t>(threads) * a.w_slots;
  T* s_rows = reinterpret_cast<T*>(s_phi + (PHI_LDS ? static_cast<size_t>(threads) * width : 0));
  const T* g_rows = static_cast<const T*>(a.rows);
  for (long long base = static_cast<long long>(blockIdx.x) * threads; base < a.n;
       base += static_cast<long long>(gridDim.x) * threads) {
    const int rows = static_cast<int>(min(static_cast<long long>(threads), a.n - base));
    if (STAGE) {
      __syncthreads();  // the previous tile's rows are no longer read
      const T* src = g_rows + base * a.ncol;
      const int nel = rows * a.ncol;
      constexpr int kPer16 = 16 / static_cast<int>(sizeof(T));
      const int nq = (reinterpret_cast<uintptr_t>(src) & 15u) == 0 ? nel / kPer16 : 0;
      const uint4* src4 = reinterpret_cast<const uint4*>(src);
      uint4* dst4 = reinterpret_cast<uint4*>(s_rows);
      for (int q = t; q < nq; q += threads) dst4[q] = src4[q];
      for (int q = nq * kPer16 + t; q < nel; q += threads) s_rows[q] = src[q];
      __syncthreads();
    }
    if (t < rows) {
      const T* row = STAGE ? s_rows + static_cast<size_t>(t) * a.ncol : g_rows + static_cast<size_t>(base + t) * a.ncol;
      double* phi = PHI_LDS ? s_phi + t : a.out + static_cast<size_t>(base + t) * width;
      const size_t ps = PHI_LDS ? threads : 1;
      for (int c = 0; c < width; ++c) phi[c * ps] = 0.0;  // this lane's own slots
      ContribRow(a.v, row, a.ncol, s_w + t, static_cast<size_t>(threads), phi, ps);
    }
    if (PHI_LDS) {
      __syncthreads();
      double* dst = a.out + static_cast<size_t>(base) * width;
      const int nel = rows * width;
      for (int q = t; q < nel; q += threads) {
        const int r = q / width, c = q - r * width;
        dst[q] = s_phi[static_cast<size_t>(c) * threads + r];
      }
      __syncthreads();  // read before the next tile's lanes zero their slots
    }
  }
}

template <typename T>
void LaunchContrib(const ContribArgs& a, const ContribShape& sh, int num_cu, hipStream_t s) {
  const long long tiles = (a.n + sh.threads - 1) / sh.threads;
  // blocks per CU by LDS (160 KiB per CU), at most 8
  const int per_cu =
      static_cast<int>(std::max<size_t>(1, std::min<size_t>(8, (size_t(160) << 10) / std::max<size_t>(1, sh.lds_bytes))));
  const int grid =
      static_cast<int>(std::max<long long>(1, std::min<long long>(tiles, static_cast<long long>(num_cu) * per_cu)));
  const size_t lds = sh.lds_bytes;
  if (sh.stage_rows) {
    if (sh.phi_lds) k_predict_contrib<T, true, true><<<grid, sh.threads, lds, s>>>(a);
    else k_predict_contrib<T, true, false><<<grid, sh.threads, lds, s>>>(a);
  } else {
    if (sh.phi_lds) k_predict_contrib<T, false, true><<<grid, sh.threads, lds, s>>>(a);
    else k_predict_contrib<T, false, false><<<grid, sh.threads, lds, s>>>(a);
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

void RequireDeviceMemory(const void* p, int dev, const char* what) {
  hipPointerAttribute_t attr{};
  const hipError_t e = hipPointerGetAttributes(&attr, p);
  if (e != hipSuccess) (void)hipGetLastError();
  if (e != hipSuccess || (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeManaged)) {
    Log::Fatal("predict_contrib_device: the %s is not GPU memory; use Booster.predict for host data", what);
  }
  if (attr.device != dev) {
    Log::Fatal("predict_contrib_device: the %s lives on GPU %d, this process predicts on GPU %d", what, attr.device,
               dev);
  }
}

}  // namespace

void PredictContribDense(const ContribPack& pack, const void* data, bool f64, int nrow, int ncol,
                         bool data_on_device, bool out_on_device, double* out) {
  if (DeviceCount() <= 0) {
    Log::Fatal("predict_device: no gfx950 GPU is visible to this process; use Booster.predict for host prediction");
  }
  if (nrow <= 0) return;
  if (ncol <= 0) Log::Fatal("predict_contrib_device: the data has no columns");
  if (pack.max_path > kCMaxPathFeatures) {
    Log::Fatal("predict_contrib_device: a path splits on %d distinct features, the kernel holds %d; use Booster.predict",
               pack.max_path, kCMaxPathFeatures);
  }
  const ContribView hv = pack.View();
  const int width = ContribWidth(hv);
  const size_t es = f64 ? 8 : 4;
  const ContribShape sh = PlanContribShape(pack.max_path, width, ncol, es);

  int dev = 0, num_cu = 256;
  HIP_CHECK(hipGetDevice(&dev));
  HIP_CHECK(hipDeviceGetAttribute(&num_cu, hipDeviceAttributeMultiprocessorCount, dev));
  if (data_on_device) RequireDeviceMemory(data, dev, "input");
  if (out_on_device) RequireDeviceMemory(out, dev, "output");
  ScopedStream st;
  hipStream_t s = st.s;

  const PackedEnsemble& pk = pack.pk;
  DevBuf<PNode> d_nodes;
  DevBuf<PTree> d_trees;
  DevBuf<int32_t> d_catb;
  DevBuf<uint32_t> d_catt;
  DevBuf<CTree> d_ctrees;
  DevBuf<CPath> d_paths;
  DevBuf<CElem> d_elems;
  DevBuf<CEdge> d_edges;
  UploadOrOne(&d_nodes, pk.nodes, s);
  UploadOrOne(&d_trees, pk.trees, s);
  UploadOrOne(&d_catb, pk.cat_boundaries, s);
  UploadOrOne(&d_catt, pk.cat_threshold, s);
  UploadOrOne(&d_ctrees, pack.ctrees, s);
  UploadOrOne(&d_paths, pack.paths, s);
  UploadOrOne(&d_elems, pack.elems, s);
  UploadOrOne(&d_edges, pack.edges, s);

  ContribArgs a{};
  a.v = hv;
  a.v.pv.nodes = d_nodes.get();
  a.v.pv.trees = d_trees.get();
  a.v.pv.cat_boundaries = d_catb.get();
  a.v.pv.cat_threshold = d_catt.get();
  a.v.pv.leaf_value = nullptr;  // ContribRow reads none of the leaf and linear arrays
  a.v.pv.lin_const = nullptr;
  a.v.pv.lin_off = nullptr;
  a.v.pv.lin_coef = nullptr;
  a.v.pv.lin_feat = nullptr;
  a.v.ctrees = d_ctrees.get();
  a.v.paths = d_paths.get();
  a.v.elems = d_elems.get();
  a.v.edges = d_edges.get();
  a.ncol = ncol;
  a.w_slots = sh.w_slots;
  a.width = width;

  // Rows in chunks of at most 256 MiB of the larger of input and output; device-resident input
  // and output are used in place, chunk by chunk.
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
    if (f64) LaunchContrib<double>(a, sh, num_cu, s);
    else LaunchContrib<float>(a, sh, num_cu, s);
    if (!out_on_device) {
      HIP_CHECK(hipMemcpyAsync(out + r0 * width, d_out.get(), out_row_bytes * rows, hipMemcpyDeviceToHost, s));
    }
  }
  HIP_CHECK(hipStreamSynchronize(s));
}

}  // namespace device
}  // namespace lgap
