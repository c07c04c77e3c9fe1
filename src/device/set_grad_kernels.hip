// Gradients and hessians supplied as device arrays (a custom objective written on the GPU,
// Booster.update_device) into the learner's layout: float2 (g, h), class-major gh[k * n + i].
// Each source is fp32 or fp64 with its own row and class stride (in elements): value (i, k) is
// src[i * rs + k * cs]. fp64 narrows with the default conversion (round to nearest even, the
// value numpy's astype(float32) gives), so the result is checkable bit for bit.
// Three kernels, chosen on the host from the strides (PlanSetGradients):
//  * rows: both row strides are 1 ((N,), class-major 1-D, (K, N).T). One streaming pass per
//    class, four rows per thread with 16-byte loads and stores where the class's three pointers
//    are 16-byte aligned, a scalar tail, and a scalar loop for a class that is not aligned;
//  * tile: both class strides are 1 and K > 1 ((N, K) contiguous, the usual torch multiclass
//    layout, and its column / row-step slices). A tile of rows x K goes through LDS as fp32:
//    lanes run along a row's classes on the read and along rows on the per-class float2 writes.
//    The LDS row stride is K made odd, so the transposed reads (stride KP dwords over a 32-lane
//    half, 32 banks for ds_read_b32) touch 32 distinct banks; the row-order writes are consecutive
//    dwords (K odd) or skip one dword per row (K even: at most 2-way where a half crosses a row);
//  * gather: anything else, one element per thread.
// Every kernel ORs "non-finite after conversion" (1: gradient, 2: hessian) into *flag: reduced
// per block, at most one atomic per block.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "device/grad_kernels.h"
#include "device/hip_common.h"

namespace lgap {
namespace device {

namespace {

constexpr int kSetThreads = 256;
constexpr int kSetMaxKP = 64;  // widest padded class count the LDS tile serves

__device__ __forceinline__ unsigned NonFinite(float g, float h) {
  constexpr unsigned e = 0x7f800000u;
  return ((__float_as_uint(g) & e) == e ? kSetGradBadGrad : 0u) | ((__float_as_uint(h) & e) == e ? kSetGradBadHess : 0u);
}

// (every thread of the block arrives here)
__device__ __forceinline__ void ReportNonFinite(unsigned bad, unsigned* __restrict__ flag) {
  const int bg = __syncthreads_or(static_cast<int>(bad & kSetGradBadGrad));
  const int bh = __syncthreads_or(static_cast<int>(bad & kSetGradBadHess));
  if (threadIdx.x == 0 && (bg != 0 || bh != 0)) atomicOr(flag, (bg ? kSetGradBadGrad : 0u) | (bh ? kSetGradBadHess : 0u));
}

// rows 4q .. 4q + 3 of a 16-byte aligned array
__device__ __forceinline__ void Load4(const float* __restrict__ p, long long q, float* out) {
  const float4 v = reinterpret_cast<const float4*>(p)[q];
  out[0] = v.x;
  out[1] = v.y;
  out[2] = v.z;
  out[3] = v.w;
}
__device__ __forceinline__ void Load4(const double* __restrict__ p, long long q, float* out) {
  const double2 a = reinterpret_cast<const double2*>(p)[2 * q], b = reinterpret_cast<const double2*>(p)[2 * q + 1];
  out[0] = static_cast<float>(a.x);
  out[1] = static_cast<float>(a.y);
  out[2] = static_cast<float>(b.x);
  out[3] = static_cast<float>(b.y);
}

template <typename Tg, typename Th>
__global__ __launch_bounds__(kSetThreads) void k_set_grad_rows(const Tg* __restrict__ g, const Th* __restrict__ h,
                                                               long long gcs, long long hcs, int n,
                                                               float2* __restrict__ gh, unsigned* __restrict__ flag) {
  const int k = blockIdx.y;
  const Tg* gk = g + k * gcs;
  const Th* hk = h + k * hcs;
  float2* o = gh + static_cast<size_t>(k) * n;
  const bool wide =
      ((reinterpret_cast<uintptr_t>(gk) | reinterpret_cast<uintptr_t>(hk) | reinterpret_cast<uintptr_t>(o)) & 15u) == 0;
  const long long quads = wide ? n / 4 : 0;
  const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
  const long long tid = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  unsigned bad = 0;
  for (long long q = tid; q < quads; q += stride) {
    float a[4], b[4];
    Load4(gk, q, a);
    Load4(hk, q, b);
#pragma unroll
    for (int j = 0; j < 4; ++j) bad |= NonFinite(a[j], b[j]);
    float4* o4 = reinterpret_cast<float4*>(o) + 2 * q;
    o4[0] = make_float4(a[0], b[0], a[1], b[1]);
    o4[1] = make_float4(a[2], b[2], a[3], b[3]);
  }
  for (long long i = quads * 4 + tid; i < n; i += stride) {
    const float a = static_cast<float>(gk[i]), b = static_cast<float>(hk[i]);
    bad |= NonFinite(a, b);
    o[i] = make_float2(a, b);
  }
  ReportNonFinite(bad, flag);
}

// R rows x K classes per tile, staged as fp32 in LDS: tg[row * KP + col], th after it
template <typename Tg, typename Th>
__global__ __launch_bounds__(kSetThreads) void k_set_grad_tile(const Tg* __restrict__ g, const Th* __restrict__ h,
                                                               long long grs, long long hrs, int n, int K, int KP, int R,
                                                               float2* __restrict__ gh, unsigned* __restrict__ flag) {
  extern __shared__ float set_grad_lds[];
  float* tg = set_grad_lds;
  float* th = set_grad_lds + R * KP;
  const int t = threadIdx.x;
  unsigned bad = 0;
  for (long long r0 = static_cast<long long>(blockIdx.x) * R; r0 < n; r0 += static_cast<long long>(gridDim.x) * R) {
    const int rows = static_cast<int>(min(static_cast<long long>(R), n - r0));
    const int cnt = rows * K;  // <= R * KP
    __syncthreads();  // the previous tile is written out
    for (int i = t; i < cnt; i += kSetThreads) {
      const int row = i / K, col = i - row * K;
      const float a = static_cast<float>(g[(r0 + row) * grs + col]);
      const float b = static_cast<float>(h[(r0 + row) * hrs + col]);
      bad |= NonFinite(a, b);
      tg[row * KP + col] = a;
      th[row * KP + col] = b;
    }
    __syncthreads();
    for (int i = t; i < cnt; i += kSetThreads) {
      const int k = i / rows, r = i - k * rows;
      gh[static_cast<size_t>(k) * n + r0 + r] = make_float2(tg[r * KP + k], th[r * KP + k]);
    }
  }
  ReportNonFinite(bad, flag);
}

template <typename Tg, typename Th>
__global__ __launch_bounds__(kSetThreads) void k_set_grad_gather(const Tg* __restrict__ g, const Th* __restrict__ h,
                                                                 long long grs, long long gcs, long long hrs, long long hcs,
                                                                 int n, int K, float2* __restrict__ gh,
                                                                 unsigned* __restrict__ flag) {
  const long long total = static_cast<long long>(n) * K;
  unsigned bad = 0;
  for (long long idx = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; idx < total;
       idx += static_cast<long long>(gridDim.x) * blockDim.x) {
    const long long k = idx / n, i = idx - k * n;
    const float a = static_cast<float>(g[i * grs + k * gcs]), b = static_cast<float>(h[i * hrs + k * hcs]);
    bad |= NonFinite(a, b);
    gh[idx] = make_float2(a, b);
  }
  ReportNonFinite(bad, flag);
}

// rows per LDS tile for a padded class count (2 x R x KP floats <= 32 KiB)
int TileRows(int KP) { return KP <= 16 ? 256 : KP <= 32 ? 128 : 64; }

template <typename Tg, typename Th>
void LaunchTyped(SetGradPath path, const GradSource& gs, const GradSource& hs, int n, int K, float2* gh, unsigned* flag,
                 int num_cu, hipStream_t s) {
  const Tg* g = static_cast<const Tg*>(gs.ptr);
  const Th* h = static_cast<const Th*>(hs.ptr);
  const int cap = std::max(1, num_cu) * 8;
  switch (path) {
    case SetGradPath::kRows: {
      const int bx = std::max(1, std::min(cap, DivUp(DivUp(n, 4), kSetThreads)));
      k_set_grad_rows<Tg, Th><<<dim3(bx, K), kSetThreads, 0, s>>>(g, h, gs.cs, hs.cs, n, gh, flag);
      break;
    }
    case SetGradPath::kTile: {
      const int KP = K | 1, R = TileRows(KP);
      const int bx = std::max(1, std::min(cap, DivUp(n, R)));
      const size_t lds = sizeof(float) * 2 * R * KP;
      k_set_grad_tile<Tg, Th><<<bx, kSetThreads, lds, s>>>(g, h, gs.rs, hs.rs, n, K, KP, R, gh, flag);
      break;
    }
    case SetGradPath::kGather: {
      const int bx = std::max(1, std::min(cap, DivUp(static_cast<long long>(n) * K, kSetThreads)));
      k_set_grad_gather<Tg, Th><<<bx, kSetThreads, 0, s>>>(g, h, gs.rs, gs.cs, hs.rs, hs.cs, n, K, gh, flag);
      break;
    }
  }
  HIP_CHECK(hipGetLastError());
}

}  // namespace

SetGradPath PlanSetGradients(const GradSource& g, const GradSource& h, int n, int num_class) {
  // (a stride is never read along a dimension of extent 1)
  const bool unit_rows = (g.rs == 1 || n == 1) && (h.rs == 1 || n == 1);
  if (unit_rows && num_class <= 65535) return SetGradPath::kRows;  // (one grid row per class)
  if (num_class > 1 && g.cs == 1 && h.cs == 1 && (num_class | 1) <= kSetMaxKP) return SetGradPath::kTile;
  return SetGradPath::kGather;
}

void LaunchSetGradients(const GradSource& g, const GradSource& h, int n, int num_class, float2* gh, unsigned* flag,
                        int num_cu, hipStream_t s) {
  if (n <= 0 || num_class <= 0) return;
  const SetGradPath path = PlanSetGradients(g, h, n, num_class);
  if (g.f64) {
    if (h.f64) LaunchTyped<double, double>(path, g, h, n, num_class, gh, flag, num_cu, s);
    else LaunchTyped<double, float>(path, g, h, n, num_class, gh, flag, num_cu, s);
  } else {
    if (h.f64) LaunchTyped<float, double>(path, g, h, n, num_class, gh, flag, num_cu, s);
    else LaunchTyped<float, float>(path, g, h, n, num_class, gh, flag, num_cu, s);
  }
}

}  // namespace device
}  // namespace lgap
