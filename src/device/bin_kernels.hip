// Feature binning on the device: a dense row-major matrix (fp32 / fp64) becomes the
// Dataset's packed group-bin rows (EFB bundles included) on the GPU.
//
// The host keeps only what needs a sample: BinMapper::FindBin and the bundle plan
// (Dataset::Construct). The per-value work — BinMapper::ValueToBin (reference
// include/LightGBM/bin.h:612-650: NaN / zero handling, binary search over the upper
// bounds, categorical lookup) and the bundle packing of Dataset::PackRows (reference
// src/io/dataset.cpp:325-441) — runs here, one thread per (row, group), so a row's
// group bytes are written by consecutive lanes; rows are staged through LDS in tiles with
// coalesced loads (k_pack_tiles), and chunk k + 1 of the matrix uploads on a copy stream
// while chunk k packs. Bundled features are applied in
// ascending column order with the host's rule (a value whose encoded bin is the
// group's zero only writes when its feature owns the group's default), so the
// result is bit-identical to the host packer.
//
// A matrix that already lives on the GPU (DevicePackResident: torch tensors as row chunks with
// element strides) is packed where it lies, without staging buffers or a copy stream: a
// contiguous row-major chunk by the same kernels, any other strides by k_pack_strided, which
// shares the pack-from-tile loop; k_gather_rows fetches the bin-construction sample.
//
// The packed rows are downloaded into the host Dataset (which stays the canonical
// container) and the device copy is kept for the HIP learner to adopt, so the
// training upload of the row-major bins is skipped.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "device/hip_common.h"
#include "lgap/common.h"
#include "lgap/dataset.h"
#include "lgap/device_api.h"
#include "lgap/log.h"

namespace lgap {
namespace device {

namespace {

struct BinFeat {
  int col;          // column of the input matrix
  int num_bin;
  int missing;      // MissingType
  int is_cat;
  int mfb, offset;  // EncodeBin
  int bounds;       // first upper bound in the flat bounds array
  int lut;          // first entry of the categorical lookup (category -> bin), -1: none
  int lut_size;
  int owner;        // this feature owns the group's template value
};

struct BinGroup {
  int first, count;  // features of the group (ascending column)
  int tmpl;          // group bin of an all-zero row
  int pad;
};

__device__ __forceinline__ uint32_t DevValueToBin(const BinFeat& f, const double* __restrict__ bounds,
                                                  const int* __restrict__ lut, double v) {
  if (v != v) {
    if (f.is_cat) return 0u;
    if (f.missing == static_cast<int>(MissingType::NaN)) return static_cast<uint32_t>(f.num_bin - 1);
    v = 0.0;
  }
  if (!f.is_cat) {
    int l = 0, r = f.num_bin - 1;
    if (f.missing == static_cast<int>(MissingType::NaN)) r -= 1;
    const double* ub = bounds + f.bounds;
    while (l < r) {
      const int m = (r + l - 1) / 2;
      if (v <= ub[m]) r = m;
      else l = m + 1;
    }
    return static_cast<uint32_t>(l);
  }
  const int iv = static_cast<int>(v);
  if (iv < 0 || iv >= f.lut_size) return 0u;
  return static_cast<uint32_t>(lut[f.lut + iv]);
}

// The group bin of one (row, group) item: the group's features applied in ascending column
// order to the row's values xr[col * cs].
template <typename T>
__device__ __forceinline__ int PackGroupBin(const T* __restrict__ xr, long long cs, const BinGroup gr,
                                            const BinFeat* __restrict__ feats, const double* __restrict__ bounds,
                                            const int* __restrict__ lut) {
  int gb = gr.tmpl;
  for (int k = 0; k < gr.count; ++k) {
    const BinFeat f = feats[gr.first + k];
    const double v = static_cast<double>(xr[f.col * cs]);
    if (!(v != v || fabs(v) > kZeroThreshold)) continue;  // zeros keep the template (host GetRow skips them)
    const uint32_t b = DevValueToBin(f, bounds, lut, v);
    const int e = b == static_cast<uint32_t>(f.mfb) ? 0 : f.offset + static_cast<int>(b) - (b > static_cast<uint32_t>(f.mfb) ? 1 : 0);
    if (e == 0 && !f.owner) continue;
    gb = e;
  }
  return gb;
}

// One thread per (row, group), values read straight from the matrix at x[row * rs + col * cs]
// (rows wider than kPackTileBytes; a contiguous matrix has rs = ncol, cs = 1).
template <typename T, int W>
__global__ __launch_bounds__(256) void k_pack_rows(const T* __restrict__ x, int nrow, long long rs, long long cs, int num_groups,
                                                   const BinGroup* __restrict__ groups, const BinFeat* __restrict__ feats,
                                                   const double* __restrict__ bounds, const int* __restrict__ lut,
                                                   int stride, uint8_t* __restrict__ out) {
  const long long total = static_cast<long long>(nrow) * num_groups;
  for (long long idx = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; idx < total;
       idx += static_cast<long long>(gridDim.x) * blockDim.x) {
    const int row = static_cast<int>(idx / num_groups);
    const int g = static_cast<int>(idx - static_cast<long long>(row) * num_groups);
    const int gb = PackGroupBin(x + static_cast<long long>(row) * rs, cs, groups[g], feats, bounds, lut);
    uint8_t* o = out + static_cast<size_t>(row) * stride;
    if (W == 1) o[g] = static_cast<uint8_t>(gb);
    else reinterpret_cast<uint16_t*>(o)[g] = static_cast<uint16_t>(gb);
  }
}

// The same packing over row tiles staged in LDS: a block loads `R` consecutive rows of the
// input matrix with coalesced 16-byte loads (the per-(row, group) kernel above reads each
// row's columns at a stride of ncol elements, one scattered access per value), then packs
// (row, group) items from LDS. The work is the binary search over a feature's upper bounds
// (~log2(num_bin) dependent loads per value, L2-resident: the per-(row, group) kernel ran
// at 97.9% L2 hit and ~0.25 TB/s), so the bounds, features and groups are staged in LDS
// too when they fit kPackTableBytes. R * ncol * sizeof(T) <= kPackTileBytes.
constexpr int kPackTileBytes = 32 * 1024;
constexpr int kPackTableBytes = 96 * 1024;
constexpr int kPackThreads = 1024;  // 16 waves per CU hide the search's LDS latency (one block per CU)

struct PackTables {
  const double* bounds;
  const BinFeat* feats;
  const BinGroup* groups;
};

// Copies the tables to the front of the block's LDS when kTables; returns the bytes they take.
// The caller's first __syncthreads() makes them visible.
template <bool kTables>
__device__ __forceinline__ size_t StagePackTables(unsigned char* lds_raw, int t, int num_groups, int nfeat, int nbounds,
                                                  PackTables* tb) {
  if (!kTables) return 0;
  double* sb = reinterpret_cast<double*>(lds_raw);
  for (int i = t; i < nbounds; i += kPackThreads) sb[i] = tb->bounds[i];
  size_t off = (sizeof(double) * nbounds + 15) & ~size_t(15);
  BinFeat* sf = reinterpret_cast<BinFeat*>(lds_raw + off);
  for (int i = t; i < nfeat * static_cast<int>(sizeof(BinFeat) / 4); i += kPackThreads) {
    reinterpret_cast<int*>(sf)[i] = reinterpret_cast<const int*>(tb->feats)[i];
  }
  off += (sizeof(BinFeat) * nfeat + 15) & ~size_t(15);
  BinGroup* sg = reinterpret_cast<BinGroup*>(lds_raw + off);
  for (int i = t; i < num_groups * static_cast<int>(sizeof(BinGroup) / 4); i += kPackThreads) {
    reinterpret_cast<int*>(sg)[i] = reinterpret_cast<const int*>(tb->groups)[i];
  }
  off += (sizeof(BinGroup) * num_groups + 15) & ~size_t(15);
  tb->bounds = sb;
  tb->feats = sf;
  tb->groups = sg;
  return off;
}

// Packs the (row, group) items of a staged row-major tile [rows x ncol]; out_rows is the packed
// row of the tile's first row.
template <typename T, int W>
__device__ __forceinline__ void PackFromTile(const T* __restrict__ tile, int rows, int ncol, int num_groups,
                                             const PackTables& tb, const int* __restrict__ lut, int stride,
                                             uint8_t* __restrict__ out_rows, int t) {
  const int items = rows * num_groups;
  for (int it = t; it < items; it += kPackThreads) {
    const int row = it / num_groups;
    const int g = it - row * num_groups;
    const int gb = PackGroupBin(tile + static_cast<size_t>(row) * ncol, 1, tb.groups[g], tb.feats, tb.bounds, lut);
    uint8_t* o = out_rows + static_cast<size_t>(row) * stride;
    if (W == 1) o[g] = static_cast<uint8_t>(gb);
    else reinterpret_cast<uint16_t*>(o)[g] = static_cast<uint16_t>(gb);
  }
}

template <typename T, int W, bool kTables>
__global__ __launch_bounds__(kPackThreads) void k_pack_tiles(const T* __restrict__ x, int nrow, int ncol, int num_groups, int R,
                                                    const BinGroup* __restrict__ groups_g, const BinFeat* __restrict__ feats_g,
                                                    int nfeat, const double* __restrict__ bounds_g, int nbounds,
                                                    const int* __restrict__ lut, int stride, uint8_t* __restrict__ out) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int t = threadIdx.x;
  PackTables tb{bounds_g, feats_g, groups_g};
  const size_t off = StagePackTables<kTables>(lds_raw, t, num_groups, nfeat, nbounds, &tb);
  T* tile = reinterpret_cast<T*>(lds_raw + off);
  for (long long r0 = static_cast<long long>(blockIdx.x) * R; r0 < nrow; r0 += static_cast<long long>(gridDim.x) * R) {
    const int rows = static_cast<int>(min(static_cast<long long>(R), nrow - r0));
    const long long n = static_cast<long long>(rows) * ncol;
    const T* src = x + r0 * ncol;
    __syncthreads();  // the previous tile's items are packed (first pass: the tables are in place)
    constexpr int per = 16 / sizeof(T);
    const long long head = (reinterpret_cast<uintptr_t>(src) & 15u) == 0 ? n / per : 0;
    for (long long i = t; i < head; i += kPackThreads) reinterpret_cast<uint4*>(tile)[i] = reinterpret_cast<const uint4*>(src)[i];
    for (long long i = head * per + t; i < n; i += kPackThreads) tile[i] = src[i];
    __syncthreads();
    PackFromTile<T, W>(tile, rows, ncol, num_groups, tb, lut, stride, out + static_cast<size_t>(r0) * stride, t);
  }
}

// k_pack_tiles for a strided view of device memory (a column slice, a row-step view, a
// transposed matrix): value (row, col) is x[row * rs + col * cs]. The tile staged in LDS is the
// same row-major [rows x ncol] image, so the packing is shared; only the load differs.
// Consecutive lanes run along the unit stride: along a row's columns (kRowLanes = false: cs = 1,
// or neither stride is 1), or along the rows of one column (kRowLanes = true: rs = 1, a
// transposed matrix), where the LDS writes are ncol elements apart.
template <typename T, int W, bool kTables, bool kRowLanes>
__global__ __launch_bounds__(kPackThreads) void k_pack_strided(const T* __restrict__ x, int nrow, int ncol, long long rs,
                                                      long long cs, int num_groups, int R,
                                                      const BinGroup* __restrict__ groups_g, const BinFeat* __restrict__ feats_g,
                                                      int nfeat, const double* __restrict__ bounds_g, int nbounds,
                                                      const int* __restrict__ lut, int stride, uint8_t* __restrict__ out) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int t = threadIdx.x;
  PackTables tb{bounds_g, feats_g, groups_g};
  const size_t off = StagePackTables<kTables>(lds_raw, t, num_groups, nfeat, nbounds, &tb);
  T* tile = reinterpret_cast<T*>(lds_raw + off);
  for (long long r0 = static_cast<long long>(blockIdx.x) * R; r0 < nrow; r0 += static_cast<long long>(gridDim.x) * R) {
    const int rows = static_cast<int>(min(static_cast<long long>(R), nrow - r0));
    const int n = rows * ncol;  // <= kPackTileBytes / sizeof(T)
    const T* src = x + r0 * rs;
    __syncthreads();  // the previous tile's items are packed (first pass: the tables are in place)
    for (int i = t; i < n; i += kPackThreads) {
      int row, col;
      if (kRowLanes) {
        col = i / rows;
        row = i - col * rows;
      } else {
        row = i / ncol;
        col = i - row * ncol;
      }
      tile[row * ncol + col] = src[row * rs + col * cs];
    }
    __syncthreads();
    PackFromTile<T, W>(tile, rows, ncol, num_groups, tb, lut, stride, out + static_cast<size_t>(r0) * stride, t);
  }
}

// Sample rows of a device-resident chunk into a contiguous row-major matrix (the
// bin-construction sample, and the whole matrix in blocks for the host fallback): item i reads
// chunk row local_rows[i] (null: first_row + i) and writes output row out_pos[i] (null:
// out_first + i). Lanes run along the source's unit stride: along the columns of a row
// (kRowLanes = false) or, for a transposed chunk (rs = 1), along the items of one column.
template <typename T, bool kRowLanes>
__global__ __launch_bounds__(256) void k_gather_rows(const T* __restrict__ x, long long rs, long long cs,
                                                     const int* __restrict__ local_rows, long long first_row,
                                                     const int* __restrict__ out_pos, long long out_first, long long n,
                                                     int ncol, T* __restrict__ out) {
  const long long total = n * ncol;
  for (long long idx = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; idx < total;
       idx += static_cast<long long>(gridDim.x) * blockDim.x) {
    long long i, col;
    if (kRowLanes) {
      col = idx / n;
      i = idx - col * n;
    } else {
      i = idx / ncol;
      col = idx - i * ncol;
    }
    const long long r = local_rows != nullptr ? local_rows[i] : first_row + i;
    const long long o = out_pos != nullptr ? out_pos[i] : out_first + i;
    out[o * ncol + col] = x[r * rs + col * cs];
  }
}

template <typename T, int W, bool kTables>
void LaunchPackTiles(dim3 grid, size_t lds, const T* x, int rows, int ncol, int G, int R, const BinGroup* groups,
                     const BinFeat* feats, int nfeat, const double* bounds, int nbounds, const int* lut, int stride,
                     uint8_t* dst, hipStream_t s) {
  if (lds > 64 * 1024) {
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_pack_tiles<T, W, kTables>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
  }
  k_pack_tiles<T, W, kTables><<<grid, kPackThreads, lds, s>>>(x, rows, ncol, G, R, groups, feats, nfeat, bounds, nbounds, lut,
                                                     stride, dst);
}

template <typename T, int W, bool kTables, bool kRowLanes>
void LaunchPackStrided(dim3 grid, size_t lds, const T* x, int rows, int ncol, long long rs, long long cs, int G, int R,
                       const BinGroup* groups, const BinFeat* feats, int nfeat, const double* bounds, int nbounds,
                       const int* lut, int stride, uint8_t* dst, hipStream_t s) {
  if (lds > 64 * 1024) {
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_pack_strided<T, W, kTables, kRowLanes>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
  }
  k_pack_strided<T, W, kTables, kRowLanes><<<grid, kPackThreads, lds, s>>>(x, rows, ncol, rs, cs, G, R, groups, feats, nfeat,
                                                                         bounds, nbounds, lut, stride, dst);
}

template <typename T, int W, bool kTables>
void LaunchPackStridedLanes(bool row_lanes, dim3 grid, size_t lds, const T* x, int rows, int ncol, long long rs, long long cs,
                            int G, int R, const BinGroup* groups, const BinFeat* feats, int nfeat, const double* bounds,
                            int nbounds, const int* lut, int stride, uint8_t* dst, hipStream_t s) {
  if (row_lanes) {
    LaunchPackStrided<T, W, kTables, true>(grid, lds, x, rows, ncol, rs, cs, G, R, groups, feats, nfeat, bounds, nbounds, lut,
                                           stride, dst, s);
  } else {
    LaunchPackStrided<T, W, kTables, false>(grid, lds, x, rows, ncol, rs, cs, G, R, groups, feats, nfeat, bounds, nbounds, lut,
                                            stride, dst, s);
  }
}

// Packs `rows` rows of x (value (i, j) at x[i * rs + j * cs]; a contiguous row-major matrix
// has rs = ncol, cs = 1) into dst.
template <typename T>
void LaunchPack(const T* x, int rows, int ncol, long long rs, long long cs, int G, int W, const BinGroup* groups,
                const BinFeat* feats, int nfeat, const double* bounds, int nbounds, const int* lut, int stride, uint8_t* dst,
                int num_cu, hipStream_t s) {
  const size_t row_bytes = sizeof(T) * static_cast<size_t>(ncol);
  const bool contiguous = (cs == 1 || ncol == 1) && (rs == ncol || rows == 1);
  if (row_bytes <= static_cast<size_t>(kPackTileBytes)) {
    const int R = static_cast<int>(std::min<size_t>(1024, kPackTileBytes / row_bytes));
    const size_t tables = ((sizeof(double) * nbounds + 15) & ~size_t(15)) + ((sizeof(BinFeat) * nfeat + 15) & ~size_t(15)) +
                          ((sizeof(BinGroup) * G + 15) & ~size_t(15));
    const bool staged = tables <= static_cast<size_t>(kPackTableBytes);
    const size_t lds = row_bytes * R + (staged ? tables : 0);
    const int grid = std::max(1, std::min(DivUp(rows, R), num_cu * (staged ? 1 : 4)));
    if (contiguous) {
      if (staged) {
        if (W == 1) LaunchPackTiles<T, 1, true>(grid, lds, x, rows, ncol, G, R, groups, feats, nfeat, bounds, nbounds, lut, stride, dst, s);
        else LaunchPackTiles<T, 2, true>(grid, lds, x, rows, ncol, G, R, groups, feats, nfeat, bounds, nbounds, lut, stride, dst, s);
      } else {
        if (W == 1) LaunchPackTiles<T, 1, false>(grid, lds, x, rows, ncol, G, R, groups, feats, nfeat, bounds, nbounds, lut, stride, dst, s);
        else LaunchPackTiles<T, 2, false>(grid, lds, x, rows, ncol, G, R, groups, feats, nfeat, bounds, nbounds, lut, stride, dst, s);
      }
    } else {
      const bool row_lanes = cs != 1 && rs == 1;
      if (staged) {
        if (W == 1) LaunchPackStridedLanes<T, 1, true>(row_lanes, grid, lds, x, rows, ncol, rs, cs, G, R, groups, feats, nfeat, bounds, nbounds, lut, stride, dst, s);
        else LaunchPackStridedLanes<T, 2, true>(row_lanes, grid, lds, x, rows, ncol, rs, cs, G, R, groups, feats, nfeat, bounds, nbounds, lut, stride, dst, s);
      } else {
        if (W == 1) LaunchPackStridedLanes<T, 1, false>(row_lanes, grid, lds, x, rows, ncol, rs, cs, G, R, groups, feats, nfeat, bounds, nbounds, lut, stride, dst, s);
        else LaunchPackStridedLanes<T, 2, false>(row_lanes, grid, lds, x, rows, ncol, rs, cs, G, R, groups, feats, nfeat, bounds, nbounds, lut, stride, dst, s);
      }
    }
  } else {
    const long long work = static_cast<long long>(rows) * G;
    const int grid = static_cast<int>(std::max<long long>(1, std::min<long long>(65536, (work + 255) / 256)));
    if (W == 1) k_pack_rows<T, 1><<<grid, 256, 0, s>>>(x, rows, rs, cs, G, groups, feats, bounds, lut, stride, dst);
    else k_pack_rows<T, 2><<<grid, 256, 0, s>>>(x, rows, rs, cs, G, groups, feats, bounds, lut, stride, dst);
  }
  HIP_CHECK(hipGetLastError());
}

// padding bytes of each packed row (stride beyond num_groups * width) are zero
__global__ void k_zero_pad(uint8_t* out, int nrow, int stride, int used) {
  const int pad = stride - used;
  for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < static_cast<long long>(nrow) * pad;
       i += static_cast<long long>(gridDim.x) * blockDim.x) {
    const long long r = i / pad;
    out[r * stride + used + (i - r * pad)] = 0;
  }
}

// Device packed rows kept for the learner, keyed by the Dataset they belong to.
struct KeptRows {
  void* ptr = nullptr;
  size_t bytes = 0;
};
std::mutex g_kept_mu;
std::map<const Dataset*, KeptRows> g_kept;

// The packing plan on the host: groups -> features in ascending column order, flat bounds,
// categorical lookups.
struct PackPlan {
  std::vector<BinGroup> groups;
  std::vector<BinFeat> feats;
  std::vector<double> bounds;
  std::vector<int> lut;
};

// False (with the reason in *why_not): a layout the device packer leaves to the host.
bool BuildPackPlan(const Dataset& ds, int ncol, PackPlan* plan, std::string* why_not) {
  const int G = ds.num_groups();
  // plan: groups -> features in ascending column order, flat bounds, categorical lookups
  std::vector<BinGroup>& groups = plan->groups;
  std::vector<BinFeat>& feats = plan->feats;
  std::vector<double>& bounds = plan->bounds;
  std::vector<int>& lut = plan->lut;
  groups.assign(std::max(G, 1), BinGroup());
  feats.clear();
  bounds.clear();
  lut.clear();
  std::vector<int> owner(G, -1);
  std::vector<int> tmpl(G, 0);
  for (int f = 0; f < ds.num_features(); ++f) {
    const FeatureInfo& fi = ds.feature(f);
    if (fi.default_bin != fi.mfb) {
      tmpl[fi.group] = Dataset::EncodeBin(fi, fi.default_bin);
      owner[fi.group] = f;
    }
  }
  for (int g = 0; g < G; ++g) {
    std::vector<int> fs = ds.group(g).features;
    std::sort(fs.begin(), fs.end(), [&](int a, int b) { return ds.feature(a).real_index < ds.feature(b).real_index; });
    groups[g].first = static_cast<int>(feats.size());
    groups[g].count = static_cast<int>(fs.size());
    groups[g].tmpl = tmpl[g];
    groups[g].pad = 0;
    for (int f : fs) {
      const FeatureInfo& fi = ds.feature(f);
      const BinMapper& m = ds.inner_mapper(f);
      if (fi.real_index >= ncol) {
        if (why_not) *why_not = "a binned feature lies beyond the matrix's columns";
        return false;
      }
      BinFeat b;
      b.col = fi.real_index;
      b.num_bin = m.num_bin();
      b.missing = static_cast<int>(m.missing_type());
      b.is_cat = m.bin_type() == BinType::Categorical ? 1 : 0;
      b.mfb = static_cast<int>(fi.mfb);
      b.offset = fi.offset;
      b.bounds = static_cast<int>(bounds.size());
      b.lut = -1;
      b.lut_size = 0;
      b.owner = owner[g] == f ? 1 : 0;
      if (b.is_cat) {
        const auto& b2c = m.bin_to_category();
        int mx = 0;
        for (int c : b2c) mx = std::max(mx, c);
        if (mx > (1 << 22)) {  // sparse huge category ids: the host map handles them
          if (why_not) *why_not = "a categorical feature has ids above 2^22";
          return false;
        }
        b.lut = static_cast<int>(lut.size());
        b.lut_size = mx + 1;
        lut.resize(lut.size() + mx + 1, 0);
        for (size_t k = 0; k < b2c.size(); ++k) {
          if (b2c[k] >= 0) lut[b.lut + b2c[k]] = static_cast<int>(k);
        }
        // bins absent from bin_to_category map to 0 as the host's cat_2_bin miss
      } else {
        const auto& ub = m.upper_bounds();
        bounds.insert(bounds.end(), ub.begin(), ub.end());
      }
      feats.push_back(b);
    }
  }
  if (feats.empty()) feats.resize(1);
  if (bounds.empty()) bounds.resize(1);
  if (lut.empty()) lut.resize(1);
  return true;
}

struct PackPlanDev {
  DevBuf<BinGroup> groups;
  DevBuf<BinFeat> feats;
  DevBuf<double> bounds;
  DevBuf<int> lut;
  void Upload(const PackPlan& p, hipStream_t s) {
    groups.Upload(p.groups, s);
    feats.Upload(p.feats, s);
    bounds.Upload(p.bounds, s);
    lut.Upload(p.lut, s);
  }
};

int NumComputeUnits() {
  int dev = 0, num_cu = 256;
  HIP_CHECK(hipGetDevice(&dev));
  HIP_CHECK(hipDeviceGetAttribute(&num_cu, hipDeviceAttributeMultiprocessorCount, dev));
  return num_cu;
}

// zeroes the packed rows' padding and queues their download
void DownloadPacked(void* d_out, int nrow, int stride, int used, uint8_t* host_out, hipStream_t s) {
  if (stride > used) {
    k_zero_pad<<<1024, 256, 0, s>>>(static_cast<uint8_t*>(d_out), nrow, stride, used);
    HIP_CHECK(hipGetLastError());
  }
  const size_t out_bytes = static_cast<size_t>(nrow) * stride;
  for (size_t off = 0; off < out_bytes; off += size_t(1) << 30) {
    HIP_CHECK(hipMemcpyAsync(host_out + off, static_cast<uint8_t*>(d_out) + off, std::min(size_t(1) << 30, out_bytes - off),
                             hipMemcpyDeviceToHost, s));
  }
}

// the packed device rows stay registered for ds's learner, or are freed
void KeepOrFree(const Dataset& ds, void* d_out, size_t out_bytes, bool keep_device_copy) {
  if (keep_device_copy) {
    std::lock_guard<std::mutex> lock(g_kept_mu);
    KeptRows& k = g_kept[&ds];
    if (k.ptr) (void)hipFree(k.ptr);
    k.ptr = d_out;
    k.bytes = out_bytes;
  } else {
    HIP_CHECK(hipFree(d_out));
  }
}

}  // namespace

bool DevicePackDense(const Dataset& ds, const void* data, bool f64, int nrow, int ncol, uint8_t* host_out,
                     bool keep_device_copy) {
  if (DeviceCount() <= 0 || nrow <= 0) return false;
  ScopedTimer timer("Device::PackRows");
  const int G = ds.num_groups();
  const int W = ds.bin_width();
  const int stride = ds.row_stride();
  PackPlan plan;
  if (!BuildPackPlan(ds, ncol, &plan, nullptr)) return false;
  // two streams: chunk k + 1 uploads (copy stream) while chunk k packs (compute stream)
  hipStream_t s, cs;
  HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  HIP_CHECK(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
  hipEvent_t up[2], packed[2];
  for (int i = 0; i < 2; ++i) {
    HIP_CHECK(hipEventCreateWithFlags(&up[i], hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&packed[i], hipEventDisableTiming));
  }
  PackPlanDev d;
  d.Upload(plan, s);
  const int nfeat = static_cast<int>(plan.feats.size()), nbounds = static_cast<int>(plan.bounds.size());
  const size_t out_bytes = static_cast<size_t>(nrow) * stride;
  void* d_out = nullptr;
  HIP_CHECK(hipMalloc(&d_out, std::max<size_t>(out_bytes, 1)));
  const int num_cu = NumComputeUnits();
  // the matrix in row chunks of <= 256 MiB, double-buffered
  const size_t es = f64 ? 8 : 4;
  const size_t row_bytes = es * static_cast<size_t>(ncol);
  const int chunk = static_cast<int>(std::max<size_t>(1, std::min<size_t>(nrow, (size_t(256) << 20) / std::max<size_t>(row_bytes, 1))));
  DevBuf<char> d_in[2];
  d_in[0].Resize(row_bytes * chunk);
  if (nrow > chunk) d_in[1].Resize(row_bytes * chunk);
  int slot = 0, n_chunk = 0;
  for (int r0 = 0; r0 < nrow; r0 += chunk, slot ^= 1, ++n_chunk) {
    const int rows = std::min(chunk, nrow - r0);
    const char* src = static_cast<const char*>(data) + row_bytes * r0;
    // the slot's previous chunk must be packed before it is overwritten
    if (n_chunk >= 2) HIP_CHECK(hipStreamWaitEvent(cs, packed[slot], 0));
    HIP_CHECK(hipMemcpyAsync(d_in[slot].get(), src, row_bytes * rows, hipMemcpyHostToDevice, cs));
    HIP_CHECK(hipEventRecord(up[slot], cs));
    HIP_CHECK(hipStreamWaitEvent(s, up[slot], 0));
    uint8_t* dst = static_cast<uint8_t*>(d_out) + static_cast<size_t>(r0) * stride;
    if (f64) {
      LaunchPack(reinterpret_cast<const double*>(d_in[slot].get()), rows, ncol, ncol, 1, G, W, d.groups.get(), d.feats.get(),
                 nfeat, d.bounds.get(), nbounds, d.lut.get(), stride, dst, num_cu, s);
    } else {
      LaunchPack(reinterpret_cast<const float*>(d_in[slot].get()), rows, ncol, ncol, 1, G, W, d.groups.get(), d.feats.get(),
                 nfeat, d.bounds.get(), nbounds, d.lut.get(), stride, dst, num_cu, s);
    }
    HIP_CHECK(hipEventRecord(packed[slot], s));
  }
  DownloadPacked(d_out, nrow, stride, G * W, host_out, s);
  HIP_CHECK(hipStreamSynchronize(s));
  HIP_CHECK(hipStreamSynchronize(cs));
  for (int i = 0; i < 2; ++i) {
    HIP_CHECK(hipEventDestroy(up[i]));
    HIP_CHECK(hipEventDestroy(packed[i]));
  }
  HIP_CHECK(hipStreamDestroy(cs));
  HIP_CHECK(hipStreamDestroy(s));
  KeepOrFree(ds, d_out, out_bytes, keep_device_copy);
  return true;
}

namespace {

struct PackStream {
  hipStream_t s = nullptr;
  PackStream() { HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
  ~PackStream() {
    if (s) (void)hipStreamDestroy(s);
  }
};

// Every chunk must be memory of the current device: a kernel reading anything else faults.
void RequireResident(const StridedChunk* chunks, int nchunk) {
  if (DeviceCount() <= 0) {
    Log::Fatal("Dataset from GPU tensors: no gfx950 GPU is visible to this process; pass host arrays instead");
  }
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  for (int c = 0; c < nchunk; ++c) {
    if (chunks[c].nrow <= 0) continue;
    hipPointerAttribute_t attr{};
    const hipError_t e = hipPointerGetAttributes(&attr, chunks[c].data);
    if (e != hipSuccess) (void)hipGetLastError();
    if (e != hipSuccess || (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeManaged)) {
      Log::Fatal("Dataset from GPU tensors: chunk %d is not GPU memory", c);
    }
    if (attr.device != dev) {
      Log::Fatal("Dataset from GPU tensors: chunk %d lives on GPU %d, this process trains on GPU %d", c, attr.device, dev);
    }
  }
}

template <typename T>
void LaunchGather(const StridedChunk& c, const int* local_rows, long long first_row, const int* out_pos, long long out_first,
                  long long n, int ncol, void* out, hipStream_t s) {
  if (n <= 0) return;
  const long long total = n * ncol;
  const int grid = static_cast<int>(std::max<long long>(1, std::min<long long>(65536, (total + 255) / 256)));
  const T* x = static_cast<const T*>(c.data);
  if (c.col_stride != 1 && c.row_stride == 1) {
    k_gather_rows<T, true><<<grid, 256, 0, s>>>(x, c.row_stride, c.col_stride, local_rows, first_row, out_pos, out_first, n,
                                                ncol, static_cast<T*>(out));
  } else {
    k_gather_rows<T, false><<<grid, 256, 0, s>>>(x, c.row_stride, c.col_stride, local_rows, first_row, out_pos, out_first, n,
                                                 ncol, static_cast<T*>(out));
  }
  HIP_CHECK(hipGetLastError());
}

void LaunchGather(bool f64, const StridedChunk& c, const int* local_rows, long long first_row, const int* out_pos,
                  long long out_first, long long n, int ncol, void* out, hipStream_t s) {
  if (f64) LaunchGather<double>(c, local_rows, first_row, out_pos, out_first, n, ncol, out, s);
  else LaunchGather<float>(c, local_rows, first_row, out_pos, out_first, n, ncol, out, s);
}

}  // namespace

bool DevicePackResident(const Dataset& ds, const StridedChunk* chunks, int nchunk, bool f64, int ncol, uint8_t* host_out,
                        bool keep_device_copy, std::string* why_not) {
  RequireResident(chunks, nchunk);
  long long total = 0;
  for (int c = 0; c < nchunk; ++c) total += chunks[c].nrow;
  if (total != ds.num_data()) Log::Fatal("Dataset from GPU tensors: %lld rows given, the dataset has %d", total, ds.num_data());
  const int nrow = static_cast<int>(total);
  if (nrow <= 0) {
    if (why_not) *why_not = "the matrix has no rows";
    return false;
  }
  PackPlan plan;
  if (!BuildPackPlan(ds, ncol, &plan, why_not)) return false;
  ScopedTimer timer("Device::PackResident");
  const int G = ds.num_groups();
  const int W = ds.bin_width();
  const int stride = ds.row_stride();
  PackStream st;
  hipStream_t s = st.s;
  PackPlanDev d;
  d.Upload(plan, s);
  const int nfeat = static_cast<int>(plan.feats.size()), nbounds = static_cast<int>(plan.bounds.size());
  const size_t out_bytes = static_cast<size_t>(nrow) * stride;
  void* d_out = nullptr;
  HIP_CHECK(hipMalloc(&d_out, std::max<size_t>(out_bytes, 1)));
  const int num_cu = NumComputeUnits();
  // every chunk is read where it lies
  size_t r0 = 0;
  for (int c = 0; c < nchunk; ++c) {
    const StridedChunk& ch = chunks[c];
    if (ch.nrow <= 0) continue;
    uint8_t* dst = static_cast<uint8_t*>(d_out) + r0 * stride;
    if (f64) {
      LaunchPack(static_cast<const double*>(ch.data), ch.nrow, ncol, ch.row_stride, ch.col_stride, G, W, d.groups.get(),
                 d.feats.get(), nfeat, d.bounds.get(), nbounds, d.lut.get(), stride, dst, num_cu, s);
    } else {
      LaunchPack(static_cast<const float*>(ch.data), ch.nrow, ncol, ch.row_stride, ch.col_stride, G, W, d.groups.get(),
                 d.feats.get(), nfeat, d.bounds.get(), nbounds, d.lut.get(), stride, dst, num_cu, s);
    }
    r0 += ch.nrow;
  }
  DownloadPacked(d_out, nrow, stride, G * W, host_out, s);
  HIP_CHECK(hipStreamSynchronize(s));
  KeepOrFree(ds, d_out, out_bytes, keep_device_copy);
  return true;
}

void GatherDeviceRows(const StridedChunk* chunks, int nchunk, bool f64, int ncol, const int* rows, long long first_row,
                      long long n, void* host_out) {
  RequireResident(chunks, nchunk);
  if (n <= 0) return;
  std::vector<long long> starts(nchunk + 1, 0);
  for (int c = 0; c < nchunk; ++c) starts[c + 1] = starts[c] + std::max(chunks[c].nrow, 0);
  const size_t row_bytes = (f64 ? 8 : 4) * static_cast<size_t>(ncol);
  PackStream st;
  hipStream_t s = st.s;
  if (rows != nullptr) {
    // the sample: resolve the global row numbers to (chunk, local row) and gather per chunk
    ScopedTimer timer("Device::GatherRows");
    std::vector<std::vector<int>> local(nchunk), pos(nchunk);
    for (long long i = 0; i < n; ++i) {
      const long long r = rows[i];
      if (r < 0 || r >= starts[nchunk]) Log::Fatal("Sampled row %lld is outside the data (%lld rows)", r, starts[nchunk]);
      const int c = static_cast<int>(std::upper_bound(starts.begin(), starts.end(), r) - starts.begin()) - 1;
      local[c].push_back(static_cast<int>(r - starts[c]));
      pos[c].push_back(static_cast<int>(i));
    }
    std::vector<int> flat_local, flat_pos;
    for (int c = 0; c < nchunk; ++c) {
      flat_local.insert(flat_local.end(), local[c].begin(), local[c].end());
      flat_pos.insert(flat_pos.end(), pos[c].begin(), pos[c].end());
    }
    DevBuf<int> d_local, d_pos;
    d_local.Upload(flat_local, s);
    d_pos.Upload(flat_pos, s);
    DevBuf<char> d_out(row_bytes * static_cast<size_t>(n));
    size_t off = 0;
    for (int c = 0; c < nchunk; ++c) {
      LaunchGather(f64, chunks[c], d_local.get() + off, 0, d_pos.get() + off, 0, static_cast<long long>(local[c].size()),
                   ncol, d_out.get(), s);
      off += local[c].size();
    }
    d_out.Download(static_cast<char*>(host_out), row_bytes * static_cast<size_t>(n), s);
    HIP_CHECK(hipStreamSynchronize(s));
    return;
  }
  // a row range (the host fallback's copy of the whole matrix): de-strided in blocks of <= 256 MiB
  ScopedTimer timer("Device::CopyRowsToHost");
  if (first_row < 0 || first_row + n > starts[nchunk]) Log::Fatal("Row range outside the data");
  const long long block = std::max<long long>(1, std::min<long long>(n, (size_t(256) << 20) / row_bytes));
  DevBuf<char> d_out(row_bytes * static_cast<size_t>(block));
  for (long long b0 = first_row; b0 < first_row + n; b0 += block) {
    const long long b1 = std::min(first_row + n, b0 + block);
    for (int c = 0; c < nchunk; ++c) {
      const long long lo = std::max(b0, starts[c]), hi = std::min(b1, starts[c + 1]);
      if (lo >= hi) continue;
      LaunchGather(f64, chunks[c], nullptr, lo - starts[c], nullptr, lo - b0, hi - lo, ncol, d_out.get(), s);
    }
    HIP_CHECK(hipMemcpyAsync(static_cast<char*>(host_out) + row_bytes * static_cast<size_t>(b0 - first_row), d_out.get(),
                             row_bytes * static_cast<size_t>(b1 - b0), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));  // the block buffer is reused
  }
}

void* TakeDeviceRows(const Dataset* ds, size_t bytes) {
  std::lock_guard<std::mutex> lock(g_kept_mu);
  auto it = g_kept.find(ds);
  if (it == g_kept.end()) return nullptr;
  void* p = it->second.ptr;
  const size_t b = it->second.bytes;
  g_kept.erase(it);
  if (b != bytes) {  // the dataset changed after packing: not usable
    (void)hipFree(p);
    return nullptr;
  }
  return p;
}

void ReleaseDeviceRows(const Dataset* ds) {
  std::lock_guard<std::mutex> lock(g_kept_mu);
  auto it = g_kept.find(ds);
  if (it == g_kept.end()) return;
  (void)hipFree(it->second.ptr);
  g_kept.erase(it);
}

}  // namespace device
}  // namespace lgap
