// Multi-tensor f32 <-> bf16 casts for gfx950.
//
// Under bf16 autocast every conv weight (an f32 master parameter that the
// optimizer changes each step) is cast to bf16 by its own launch in
// forward, and every weight gradient back to f32 by its own launch in
// backward: ResNet50 spends 106 launches of about 5 us on a few hundred
// KB each. These two kernels cast a whole list per launch, built the way
// sgd_mom_multi_f32_kernel (ks_ops.hip) is: pointers, element counts and
// a prefix sum of per-tensor block counts travel BY VALUE in the kernel
// arguments (4096-byte limit), so nothing requires a tensor to stay at
// the same address from call to call and the launch is capturable into
// a hipGraph. A block binary-searches the prefix sum for its tensor and
// owns one KS_CAST_CHUNK-element chunk of it.
//
// Rounding is torch's (c10::detail::round_to_nearest_even): round to
// nearest even, every NaN becomes the canonical quiet NaN 0x7FC0. The
// f32_to_bf16 helper of bn_relu.hip is NOT that (a NaN whose payload sits
// in the low mantissa bits comes out as inf there) and is not used here.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <vector>

#include "cast_common.h"

#define KS_CAST_THREADS 256
#define KS_CAST_VPT 4  // 8-element vectors per thread, all loads first
#define KS_CAST_CHUNK (KS_CAST_THREADS * KS_CAST_VPT * 8)
#define KS_CAST_MAX_TENSORS 128

typedef __attribute__((ext_vector_type(8))) unsigned short cast_ushort8;

struct CastMultiArgs {
  const void* src[KS_CAST_MAX_TENSORS];
  void* dst[KS_CAST_MAX_TENSORS];
  long long n[KS_CAST_MAX_TENSORS];
  // blk[t] = first block of tensor t; blk[count] = grid size
  int blk[KS_CAST_MAX_TENSORS + 1];
  int count;
};
static_assert(sizeof(CastMultiArgs) <= 4096,
              "CastMultiArgs must fit the 4 KiB kernel-argument segment");

// 8 elements: two float4 on the f32 side, one 16-byte vector on the
// bf16 side
struct CastF8 {
  float4 lo, hi;
};

__device__ __forceinline__ cast_ushort8 cast_pack8(const CastF8& f) {
  cast_ushort8 o;
  o[0] = cast_f32_to_bf16(f.lo.x);
  o[1] = cast_f32_to_bf16(f.lo.y);
  o[2] = cast_f32_to_bf16(f.lo.z);
  o[3] = cast_f32_to_bf16(f.lo.w);
  o[4] = cast_f32_to_bf16(f.hi.x);
  o[5] = cast_f32_to_bf16(f.hi.y);
  o[6] = cast_f32_to_bf16(f.hi.z);
  o[7] = cast_f32_to_bf16(f.hi.w);
  return o;
}

__device__ __forceinline__ CastF8 cast_unpack8(const cast_ushort8& u) {
  CastF8 f;
  f.lo = make_float4(cast_bf16_to_f32(u[0]), cast_bf16_to_f32(u[1]),
                     cast_bf16_to_f32(u[2]), cast_bf16_to_f32(u[3]));
  f.hi = make_float4(cast_bf16_to_f32(u[4]), cast_bf16_to_f32(u[5]),
                     cast_bf16_to_f32(u[6]), cast_bf16_to_f32(u[7]));
  return f;
}

// TO_BF16: src is f32 and dst bf16; otherwise src is bf16 and dst f32.
template <bool TO_BF16>
__global__ void __launch_bounds__(KS_CAST_THREADS)
cast_multi_kernel(const CastMultiArgs a) {
  const int b = blockIdx.x;
  // largest t with blk[t] <= b (blk is non-decreasing, blk[0] == 0,
  // b < blk[count]; tensors own >= 1 block, so the answer is unique)
  int lo = 0, hi = a.count - 1;
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (a.blk[mid] <= b) lo = mid; else hi = mid - 1;
  }
  const long long base = (long long)(b - a.blk[lo]) * KS_CAST_CHUNK;
  const long long rem = a.n[lo] - base;  // > 0 by construction of blk
  const int len = rem < KS_CAST_CHUNK ? (int)rem : KS_CAST_CHUNK;
  const float* __restrict__ f32p;
  const unsigned short* __restrict__ srcb;
  float* __restrict__ dstf;
  unsigned short* __restrict__ bf16p;
  if (TO_BF16) {
    f32p = static_cast<const float*>(a.src[lo]) + base;
    bf16p = static_cast<unsigned short*>(a.dst[lo]) + base;
  } else {
    srcb = static_cast<const unsigned short*>(a.src[lo]) + base;
    dstf = static_cast<float*>(a.dst[lo]) + base;
  }
  const int tid = threadIdx.x;
  // base is a multiple of 8 elements, so the chunk starts are 16-byte
  // aligned exactly when the tensor starts are; misaligned views
  // (narrow() at an odd offset) take the scalar path
  const bool vec = TO_BF16
      ? (((uintptr_t)f32p | (uintptr_t)bf16p) & 15) == 0
      : (((uintptr_t)srcb | (uintptr_t)dstf) & 15) == 0;
  if (!vec) {
    for (int k = tid; k < len; k += KS_CAST_THREADS) {
      if (TO_BF16) bf16p[k] = cast_f32_to_bf16(f32p[k]);
      else dstf[k] = cast_bf16_to_f32(srcb[k]);
    }
    return;
  }
  const int len8 = len >> 3;
  if (TO_BF16) {
    const float4* s4 = reinterpret_cast<const float4*>(f32p);
    cast_ushort8* d8 = reinterpret_cast<cast_ushort8*>(bf16p);
    if (len == KS_CAST_CHUNK) {
      CastF8 v[KS_CAST_VPT];
#pragma unroll
      for (int u = 0; u < KS_CAST_VPT; u++) {
        const int k = tid + u * KS_CAST_THREADS;
        v[u].lo = s4[2 * k];
        v[u].hi = s4[2 * k + 1];
      }
#pragma unroll
      for (int u = 0; u < KS_CAST_VPT; u++)
        d8[tid + u * KS_CAST_THREADS] = cast_pack8(v[u]);
      return;
    }
    for (int k = tid; k < len8; k += KS_CAST_THREADS) {
      CastF8 v;
      v.lo = s4[2 * k];
      v.hi = s4[2 * k + 1];
      d8[k] = cast_pack8(v);
    }
    for (int k = len8 * 8 + tid; k < len; k += KS_CAST_THREADS)
      bf16p[k] = cast_f32_to_bf16(f32p[k]);
  } else {
    const cast_ushort8* s8 = reinterpret_cast<const cast_ushort8*>(srcb);
    float4* d4 = reinterpret_cast<float4*>(dstf);
    if (len == KS_CAST_CHUNK) {
      cast_ushort8 v[KS_CAST_VPT];
#pragma unroll
      for (int u = 0; u < KS_CAST_VPT; u++)
        v[u] = s8[tid + u * KS_CAST_THREADS];
#pragma unroll
      for (int u = 0; u < KS_CAST_VPT; u++) {
        const int k = tid + u * KS_CAST_THREADS;
        const CastF8 f = cast_unpack8(v[u]);
        d4[2 * k] = f.lo;
        d4[2 * k + 1] = f.hi;
      }
      return;
    }
    for (int k = tid; k < len8; k += KS_CAST_THREADS) {
      const CastF8 f = cast_unpack8(s8[k]);
      d4[2 * k] = f.lo;
      d4[2 * k + 1] = f.hi;
    }
    for (int k = len8 * 8 + tid; k < len; k += KS_CAST_THREADS)
      dstf[k] = cast_bf16_to_f32(srcb[k]);
  }
}

namespace {

// Casts every defined entry of `src` (dtype `from`) into a new tensor of
// dtype `to` with the same sizes and strides; None entries stay None. A
// tensor the flat kernel cannot take (not dense, or not on the current
// device) goes through Tensor::to.
template <bool TO_BF16>
std::vector<c10::optional<torch::Tensor>> cast_multi(
    const std::vector<c10::optional<torch::Tensor>>& src, const char* name) {
  const auto from = TO_BF16 ? at::kFloat : at::kBFloat16;
  const auto to = TO_BF16 ? at::kBFloat16 : at::kFloat;
  auto stream = at::cuda::getCurrentCUDAStream();
  const long long max_blocks = 1LL << 30;
  CastMultiArgs a = {};
  a.count = 0;
  a.blk[0] = 0;
  auto flush = [&]() {
    if (a.count == 0) return;
    hipLaunchKernelGGL(cast_multi_kernel<TO_BF16>, dim3(a.blk[a.count]),
                       dim3(KS_CAST_THREADS), 0, stream.stream(), a);
    a.count = 0;
  };
  std::vector<c10::optional<torch::Tensor>> out(src.size());
  for (size_t t = 0; t < src.size(); t++) {
    if (!src[t].has_value() || !src[t]->defined()) continue;
    const torch::Tensor& s = *src[t];
    TORCH_CHECK(s.is_cuda() && s.scalar_type() == from, name,
                ": CUDA tensors of the source dtype expected");
    if (!s.is_non_overlapping_and_dense() ||
        s.get_device() != stream.device_index()) {
      out[t] = s.to(to);
      continue;
    }
    // same sizes and strides (dense): the cast runs over flat storage
    torch::Tensor d = at::empty_strided(s.sizes(), s.strides(),
                                        s.options().dtype(to));
    out[t] = d;
    const long long n = s.numel();
    if (n == 0) continue;
    const long long nb = (n + KS_CAST_CHUNK - 1) / KS_CAST_CHUNK;
    TORCH_CHECK(nb <= max_blocks, name, ": tensor too large");
    if (a.count == KS_CAST_MAX_TENSORS || a.blk[a.count] + nb > max_blocks)
      flush();
    a.src[a.count] = s.data_ptr();
    a.dst[a.count] = d.data_ptr();
    a.n[a.count] = n;
    a.blk[a.count + 1] = a.blk[a.count] + (int)nb;
    a.count++;
  }
  flush();
  return out;
}

}  // namespace

std::vector<c10::optional<torch::Tensor>> cast_f32_to_bf16_multi(
    std::vector<c10::optional<torch::Tensor>> src) {
  return cast_multi<true>(src, "cast_f32_to_bf16_multi");
}

std::vector<c10::optional<torch::Tensor>> cast_bf16_to_f32_multi(
    std::vector<c10::optional<torch::Tensor>> src) {
  return cast_multi<false>(src, "cast_bf16_to_f32_multi");
}

// ------------------------------------------------ mirrored conv weights
//
// mirror_weights_multi: for every bf16 weight (K,C,R,S) of a list, the
// weight of the forward convolution that computes the stride-1 data
// gradient: out[c,k,r,s] = in[k,c,R-1-r,S-1-s], (C,K,R,S), channels-last.
// In memory the source is [K][R*S][C] and the result [C][R*S][K], so each
// filter tap is a K x C -> C x K transpose between rows of R*S*C and
// R*S*K elements, tap t landing at tap R*S-1-t. A block owns one 64 x 64
// tile of one tap: it reads rows of the source (16 bytes per lane, eight
// lanes per row), turns the tile in LDS and writes rows of the result the
// same way. LDS rows are 66 elements (33 dwords, odd): the column reads
// of the second phase touch dword (8*kv + j) * 33 + c / 2 for the lane's
// k-vector kv = 0..7 and four values of c / 2, i.e. banks 8*kv + 0..3,
// all distinct. The launch is cast_multi_kernel's: pointers, K, C, R*S
// and the block prefix sum by value in the kernel arguments.
#define KS_MIRROR_THREADS 256
#define KS_MIRROR_TILE 64
#define KS_MIRROR_LD (KS_MIRROR_TILE + 2)
// 2 pointers + 4 ints per tensor, then blk[count] and count
#define KS_MIRROR_MAX_TENSORS ((4096 - 8) / 32)

struct MirrorMultiArgs {
  const void* src[KS_MIRROR_MAX_TENSORS];
  void* dst[KS_MIRROR_MAX_TENSORS];
  int K[KS_MIRROR_MAX_TENSORS];
  int C[KS_MIRROR_MAX_TENSORS];
  int RS[KS_MIRROR_MAX_TENSORS];
  // blk[t] = first block of tensor t; blk[count] = grid size
  int blk[KS_MIRROR_MAX_TENSORS + 1];
  int count;
};
static_assert(sizeof(MirrorMultiArgs) <= 4096,
              "MirrorMultiArgs must fit the 4 KiB kernel-argument segment");
static_assert(KS_MIRROR_THREADS == 4 * KS_MIRROR_TILE &&
                  KS_MIRROR_TILE % 8 == 0,
              "a block covers the tile in two passes of 32 rows, eight "
              "8-element vectors per row");

__global__ void __launch_bounds__(KS_MIRROR_THREADS)
mirror_multi_kernel(const MirrorMultiArgs a) {
  __shared__ unsigned short tile[KS_MIRROR_TILE][KS_MIRROR_LD];
  const int b = blockIdx.x;
  // largest t with blk[t] <= b, as in cast_multi_kernel
  int lo = 0, hi = a.count - 1;
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (a.blk[mid] <= b) lo = mid; else hi = mid - 1;
  }
  const int K = a.K[lo], C = a.C[lo], RS = a.RS[lo];
  const int tiles_c = (C + KS_MIRROR_TILE - 1) / KS_MIRROR_TILE;
  const int tiles_k = (K + KS_MIRROR_TILE - 1) / KS_MIRROR_TILE;
  int lb = b - a.blk[lo];  // < RS * tiles_k * tiles_c by construction
  const int c0 = (lb % tiles_c) * KS_MIRROR_TILE;
  lb /= tiles_c;
  const int k0 = (lb % tiles_k) * KS_MIRROR_TILE;
  const int tap = lb / tiles_k;
  const long long srow = (long long)RS * C, drow = (long long)RS * K;
  // element (k, c) of source tap RS-1-tap; element (c, k) of result tap
  const unsigned short* __restrict__ src =
      static_cast<const unsigned short*>(a.src[lo]) +
      (long long)(RS - 1 - tap) * C;
  unsigned short* __restrict__ dst =
      static_cast<unsigned short*>(a.dst[lo]) + (long long)tap * K;
  const int row = threadIdx.x >> 3;       // 0..31
  const int v = (threadIdx.x & 7) * 8;    // first of the lane's 8 columns
  // with C % 8 == 0 every row start and every v is a multiple of 8
  // elements: 16-byte aligned exactly when the tensor is
  const bool vin = (C & 7) == 0 && ((uintptr_t)a.src[lo] & 15) == 0;
  const bool vout = (K & 7) == 0 && ((uintptr_t)a.dst[lo] & 15) == 0;
#pragma unroll
  for (int p = 0; p < 2; p++) {
    const int k = row + p * 32;
    const int gk = k0 + k, gc = c0 + v;
    if (gk >= K) continue;
    const unsigned short* s = src + gk * srow + gc;
    if (vin) {
      if (gc < C) {  // a vector is inside or outside as a whole
        const cast_ushort8 x = *reinterpret_cast<const cast_ushort8*>(s);
#pragma unroll
        for (int j = 0; j < 8; j++) tile[k][v + j] = x[j];
      }
    } else {
      for (int j = 0; j < 8; j++)
        if (gc + j < C) tile[k][v + j] = s[j];
    }
  }
  __syncthreads();
  // only elements loaded above are read: the same bounds, transposed
#pragma unroll
  for (int p = 0; p < 2; p++) {
    const int c = row + p * 32;
    const int gc = c0 + c, gk = k0 + v;
    if (gc >= C) continue;
    unsigned short* d = dst + gc * drow + gk;
    if (vout) {
      if (gk < K) {
        cast_ushort8 o;
#pragma unroll
        for (int j = 0; j < 8; j++) o[j] = tile[v + j][c];
        *reinterpret_cast<cast_ushort8*>(d) = o;
      }
    } else {
      for (int j = 0; j < 8; j++)
        if (gk + j < K) d[j] = tile[v + j][c];
    }
  }
}

// The torch expression the kernel reproduces bit for bit.
static torch::Tensor mirror_weight_eager(const torch::Tensor& w) {
  return w.flip({2, 3}).transpose(0, 1).contiguous(
      at::MemoryFormat::ChannelsLast);
}

std::vector<torch::Tensor> mirror_weights_multi(
    std::vector<torch::Tensor> src) {
  auto stream = at::cuda::getCurrentCUDAStream();
  const long long max_blocks = 1LL << 30;
  MirrorMultiArgs a = {};
  a.count = 0;
  a.blk[0] = 0;
  auto flush = [&]() {
    if (a.count == 0) return;
    hipLaunchKernelGGL(mirror_multi_kernel, dim3(a.blk[a.count]),
                       dim3(KS_MIRROR_THREADS), 0, stream.stream(), a);
    a.count = 0;
  };
  std::vector<torch::Tensor> out(src.size());
  for (size_t t = 0; t < src.size(); t++) {
    const torch::Tensor& s = src[t];
    TORCH_CHECK(s.defined() && s.dim() == 4,
                "mirror_weights_multi: 4-d weights (K,C,R,S) expected");
    if (!s.is_cuda() || s.scalar_type() != at::kBFloat16 ||
        s.get_device() != stream.device_index() ||
        !s.is_contiguous(at::MemoryFormat::ChannelsLast)) {
      out[t] = mirror_weight_eager(s);
      continue;
    }
    const long long K = s.size(0), C = s.size(1), RS = s.size(2) * s.size(3);
    torch::Tensor d = at::empty(
        {C, K, s.size(2), s.size(3)},
        s.options().memory_format(at::MemoryFormat::ChannelsLast));
    out[t] = d;
    if (s.numel() == 0) continue;
    const long long nb = RS * ((K + KS_MIRROR_TILE - 1) / KS_MIRROR_TILE) *
                         ((C + KS_MIRROR_TILE - 1) / KS_MIRROR_TILE);
    TORCH_CHECK(s.numel() < (1LL << 31) && nb <= max_blocks,
                "mirror_weights_multi: tensor too large");
    if (a.count == KS_MIRROR_MAX_TENSORS || a.blk[a.count] + nb > max_blocks)
      flush();
    a.src[a.count] = s.data_ptr();
    a.dst[a.count] = d.data_ptr();
    a.K[a.count] = (int)K;
    a.C[a.count] = (int)C;
    a.RS[a.count] = (int)RS;
    a.blk[a.count + 1] = a.blk[a.count] + (int)nb;
    a.count++;
  }
  flush();
  return out;
}
