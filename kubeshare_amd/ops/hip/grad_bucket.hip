// Multi-tensor pack / unpack between per-parameter f32 tensors and one
// flat gradient bucket (f32 or bf16) for gfx950.
//
// A gang rank on the fused path averages its gradients with ONE
// collective over one persistent flat buffer (ops.GradBucket) instead of
// a DDP reducer: pack scales every gradient into its segment of the
// buffer, the buffer is all-reduced, and the multi-tensor SGD reads the
// segments as its gradients. Built the way cast_multi_kernel (cast.hip)
// and sgd_mom_multi_f32_kernel (ks_ops.hip) are: pointers, element
// counts and a prefix sum of per-tensor block counts travel BY VALUE in
// the kernel arguments (4096-byte limit), one launch handles up to
// KS_GB_MAX_TENSORS tensors, a block binary-searches the prefix sum for
// its tensor and owns one KS_GB_CHUNK-element chunk of it. No atomics,
// no grid-wide synchronisation: every element is written by exactly one
// thread.
//
// pack:    flat[off_t + i] = FlatT(scale * src_t[i])   (src_t f32)
// unpack:  dst_t[i]        = float(flat[off_t + i])    (dst_t f32)
//
// i runs over the flat dense storage of the tensor, in storage order,
// which is how the SGD kernel treats channels-last weights. The scale is
// one f32 multiply per element; the bf16 rounding is torch's (RNE, every
// NaN becomes 0x7FC0), so a packed segment holds the bits of
// (g * scale).to(dtype).
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <vector>

#include "cast_common.h"  // torch's bf16 rounding, NOT bn_relu.hip's

#define KS_GB_THREADS 256
#define KS_GB_VPT 4  // 8-element vectors per thread, all loads first
#define KS_GB_CHUNK (KS_GB_THREADS * KS_GB_VPT * 8)
#define KS_GB_MAX_TENSORS 128

typedef __attribute__((ext_vector_type(8))) unsigned short gb_ushort8;

struct GradBucketArgs {
  // pack: src[t] is the tensor (nullptr: zeros), dst[t] its segment of
  // the flat buffer; unpack: the other way round
  const void* src[KS_GB_MAX_TENSORS];
  void* dst[KS_GB_MAX_TENSORS];
  long long n[KS_GB_MAX_TENSORS];
  // blk[t] = first block of tensor t; blk[count] = grid size
  int blk[KS_GB_MAX_TENSORS + 1];
  int count;
  float scale;  // pack only
};
static_assert(sizeof(GradBucketArgs) <= 4096,
              "GradBucketArgs must fit the 4 KiB kernel-argument segment");

// 8 consecutive elements in registers, always as f32
struct GbF8 {
  float4 lo, hi;
};

__device__ __forceinline__ GbF8 gb_load8(const float* p, int k) {
  const float4* p4 = reinterpret_cast<const float4*>(p);
  GbF8 f;
  f.lo = p4[2 * k];
  f.hi = p4[2 * k + 1];
  return f;
}

__device__ __forceinline__ GbF8 gb_load8(const unsigned short* p, int k) {
  const gb_ushort8 u = reinterpret_cast<const gb_ushort8*>(p)[k];
  GbF8 f;
  f.lo = make_float4(cast_bf16_to_f32(u[0]), cast_bf16_to_f32(u[1]),
                     cast_bf16_to_f32(u[2]), cast_bf16_to_f32(u[3]));
  f.hi = make_float4(cast_bf16_to_f32(u[4]), cast_bf16_to_f32(u[5]),
                     cast_bf16_to_f32(u[6]), cast_bf16_to_f32(u[7]));
  return f;
}

__device__ __forceinline__ void gb_store8(float* p, int k, const GbF8& f) {
  float4* p4 = reinterpret_cast<float4*>(p);
  p4[2 * k] = f.lo;
  p4[2 * k + 1] = f.hi;
}

__device__ __forceinline__ void gb_store8(unsigned short* p, int k,
                                          const GbF8& f) {
  gb_ushort8 o;
  o[0] = cast_f32_to_bf16(f.lo.x);
  o[1] = cast_f32_to_bf16(f.lo.y);
  o[2] = cast_f32_to_bf16(f.lo.z);
  o[3] = cast_f32_to_bf16(f.lo.w);
  o[4] = cast_f32_to_bf16(f.hi.x);
  o[5] = cast_f32_to_bf16(f.hi.y);
  o[6] = cast_f32_to_bf16(f.hi.z);
  o[7] = cast_f32_to_bf16(f.hi.w);
  reinterpret_cast<gb_ushort8*>(p)[k] = o;
}

__device__ __forceinline__ float gb_load1(const float* p, int k) {
  return p[k];
}
__device__ __forceinline__ float gb_load1(const unsigned short* p, int k) {
  return cast_bf16_to_f32(p[k]);
}
__device__ __forceinline__ void gb_store1(float* p, int k, float f) {
  p[k] = f;
}
__device__ __forceinline__ void gb_store1(unsigned short* p, int k, float f) {
  p[k] = cast_f32_to_bf16(f);
}

// SCALE: multiply by a.scale (pack); an unpack moves the value as it is
template <bool SCALE>
__device__ __forceinline__ float gb_scale1(float x, float s) {
  return SCALE ? s * x : x;
}

template <bool SCALE>
__device__ __forceinline__ GbF8 gb_scale8(GbF8 f, float s) {
  if (SCALE) {
    f.lo.x = s * f.lo.x;
    f.lo.y = s * f.lo.y;
    f.lo.z = s * f.lo.z;
    f.lo.w = s * f.lo.w;
    f.hi.x = s * f.hi.x;
    f.hi.y = s * f.hi.y;
    f.hi.z = s * f.hi.z;
    f.hi.w = s * f.hi.w;
  }
  return f;
}

// PACK: SrcT is float (the tensors), DstT the bucket's element type
// (float, or unsigned short holding bf16 bits); a null source writes
// zeros. Otherwise SrcT is the bucket's type and DstT float.
template <bool PACK, typename SrcT, typename DstT>
__global__ void __launch_bounds__(KS_GB_THREADS)
grad_bucket_multi_kernel(const GradBucketArgs a) {
  const int b = blockIdx.x;
  // largest t with blk[t] <= b (blk is non-decreasing, blk[0] == 0,
  // b < blk[count]; tensors own >= 1 block, so the answer is unique)
  int lo = 0, hi = a.count - 1;
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (a.blk[mid] <= b) lo = mid; else hi = mid - 1;
  }
  const long long base = (long long)(b - a.blk[lo]) * KS_GB_CHUNK;
  const long long rem = a.n[lo] - base;  // > 0 by construction of blk
  const int len = rem < KS_GB_CHUNK ? (int)rem : KS_GB_CHUNK;
  const bool zero = PACK && a.src[lo] == nullptr;
  // (a null source is never dereferenced: every load below is behind
  // !zero)
  const SrcT* __restrict__ src =
      zero ? nullptr : static_cast<const SrcT*>(a.src[lo]) + base;
  DstT* __restrict__ dst = static_cast<DstT*>(a.dst[lo]) + base;
  const float s = a.scale;
  const int tid = threadIdx.x;
  // base is a multiple of 8 elements, so the chunk starts are 16-byte
  // aligned exactly when the tensor and its segment are; misaligned
  // views (narrow() at an odd offset) take the scalar path
  const bool vec = (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
  if (!vec) {
    for (int k = tid; k < len; k += KS_GB_THREADS)
      gb_store1(dst, k, zero ? 0.0f : gb_scale1<PACK>(gb_load1(src, k), s));
    return;
  }
  const int len8 = len >> 3;
  if (zero) {
    GbF8 z;
    z.lo = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    z.hi = z.lo;
    for (int k = tid; k < len8; k += KS_GB_THREADS) gb_store8(dst, k, z);
    for (int k = len8 * 8 + tid; k < len; k += KS_GB_THREADS)
      gb_store1(dst, k, 0.0f);
    return;
  }
  if (len == KS_GB_CHUNK) {
    GbF8 v[KS_GB_VPT];
#pragma unroll
    for (int u = 0; u < KS_GB_VPT; u++)
      v[u] = gb_load8(src, tid + u * KS_GB_THREADS);
#pragma unroll
    for (int u = 0; u < KS_GB_VPT; u++)
      gb_store8(dst, tid + u * KS_GB_THREADS, gb_scale8<PACK>(v[u], s));
    return;
  }
  for (int k = tid; k < len8; k += KS_GB_THREADS)
    gb_store8(dst, k, gb_scale8<PACK>(gb_load8(src, k), s));
  for (int k = len8 * 8 + tid; k < len; k += KS_GB_THREADS)
    gb_store1(dst, k, gb_scale1<PACK>(gb_load1(src, k), s));
}

namespace {

// Collects (src, dst, n) triples and launches them KS_GB_MAX_TENSORS at
// a time.
template <bool PACK, typename SrcT, typename DstT>
struct GbLauncher {
  GradBucketArgs a = {};
  hipStream_t stream;
  int64_t launches = 0;
  static constexpr long long max_blocks = 1LL << 30;

  GbLauncher(hipStream_t s, float scale) : stream(s) {
    a.count = 0;
    a.blk[0] = 0;
    a.scale = scale;
  }
  void flush() {
    if (a.count == 0) return;
    hipLaunchKernelGGL((grad_bucket_multi_kernel<PACK, SrcT, DstT>),
                       dim3(a.blk[a.count]), dim3(KS_GB_THREADS), 0, stream,
                       a);
    launches++;
    a.count = 0;
  }
  void add(const void* src, void* dst, long long n, const char* name) {
    if (n == 0) return;
    const long long nb = (n + KS_GB_CHUNK - 1) / KS_GB_CHUNK;
    TORCH_CHECK(nb <= max_blocks, name, ": tensor too large");
    if (a.count == KS_GB_MAX_TENSORS || a.blk[a.count] + nb > max_blocks)
      flush();
    a.src[a.count] = src;
    a.dst[a.count] = dst;
    a.n[a.count] = n;
    a.blk[a.count + 1] = a.blk[a.count] + (int)nb;
    a.count++;
  }
};

void check_flat(const torch::Tensor& flat, const char* name) {
  TORCH_CHECK(flat.is_cuda() && flat.dim() == 1 && flat.is_contiguous() &&
                  (flat.scalar_type() == at::kFloat ||
                   flat.scalar_type() == at::kBFloat16),
              name, ": the flat buffer is a contiguous 1-D f32 or bf16 CUDA "
              "tensor");
  TORCH_CHECK(flat.get_device() ==
                  at::cuda::getCurrentCUDAStream().device_index(),
              name, ": the flat buffer must live on the current device");
}

// Segment t is [offsets[t], offsets[t] + n) of flat; anything else would
// have the kernel write (pack) or read (unpack) out of bounds.
char* segment(const torch::Tensor& flat, int64_t off, long long n,
              const char* name) {
  TORCH_CHECK(off >= 0 && n >= 0 && off <= flat.numel() &&
                  n <= flat.numel() - off,
              name, ": segment [", off, ", ", off + n, ") leaves the flat "
              "buffer of ", flat.numel(), " elements");
  return static_cast<char*>(flat.data_ptr()) + off * flat.element_size();
}

template <typename FlatT>
int64_t pack_impl(const std::vector<c10::optional<torch::Tensor>>& srcs,
                  torch::Tensor& flat, const std::vector<int64_t>& offsets,
                  float scale, const std::vector<torch::Tensor>& like) {
  const char* name = "grad_pack_multi";
  auto stream = at::cuda::getCurrentCUDAStream();
  GbLauncher<true, float, FlatT> l(stream.stream(), scale);
  // re-strided source copies live until every launch is enqueued
  std::vector<torch::Tensor> keep;
  for (size_t t = 0; t < srcs.size(); t++) {
    const torch::Tensor& v = like[t];
    TORCH_CHECK(v.is_non_overlapping_and_dense(), name,
                ": segment layouts must be non-overlapping and dense");
    const long long n = v.numel();
    char* dst = segment(flat, offsets[t], n, name);
    if (!srcs[t].has_value() || !srcs[t]->defined()) {
      l.add(nullptr, dst, n, name);
      continue;
    }
    torch::Tensor s = *srcs[t];
    TORCH_CHECK(s.is_cuda() && s.scalar_type() == at::kFloat &&
                    s.sizes() == v.sizes() &&
                    s.get_device() == stream.device_index(),
                name, ": f32 tensor of the segment's shape on the current "
                "device expected");
    if (s.strides() != v.strides()) {
      // rare: e.g. a contiguous gradient for a channels-last weight
      s = at::empty_strided(v.sizes(), v.strides(), s.options()).copy_(s);
      keep.push_back(s);
    }
    l.add(s.data_ptr(), dst, n, name);
  }
  l.flush();
  return l.launches;
}

template <typename FlatT>
int64_t unpack_impl(const torch::Tensor& flat,
                    const std::vector<int64_t>& offsets,
                    const std::vector<c10::optional<torch::Tensor>>& dsts) {
  const char* name = "grad_unpack_multi";
  auto stream = at::cuda::getCurrentCUDAStream();
  GbLauncher<false, FlatT, float> l(stream.stream(), 1.0f);
  for (size_t t = 0; t < dsts.size(); t++) {
    if (!dsts[t].has_value() || !dsts[t]->defined()) continue;
    const torch::Tensor& d = *dsts[t];
    TORCH_CHECK(d.is_cuda() && d.scalar_type() == at::kFloat &&
                    d.is_non_overlapping_and_dense() &&
                    d.get_device() == stream.device_index(),
                name, ": dense f32 tensors on the current device expected");
    const long long n = d.numel();
    const char* src = segment(flat, offsets[t], n, name);
    l.add(src, d.data_ptr(), n, name);
  }
  l.flush();
  return l.launches;
}

}  // namespace

// flat[offsets[t] + i] = FlatT(f32(scale) * srcs[t][i]) over the flat
// storage of like[t]'s layout (sizes and strides of segment t: the
// bucket's views). A None source writes zeros; a source with other
// strides is re-strided first. Returns the number of kernels launched.
int64_t grad_pack_multi(std::vector<c10::optional<torch::Tensor>> srcs,
                        torch::Tensor flat, std::vector<int64_t> offsets,
                        double scale, std::vector<torch::Tensor> like) {
  check_flat(flat, "grad_pack_multi");
  TORCH_CHECK(srcs.size() == offsets.size() && srcs.size() == like.size(),
              "grad_pack_multi: srcs, offsets and like differ in length");
  if (flat.scalar_type() == at::kFloat)
    return pack_impl<float>(srcs, flat, offsets, (float)scale, like);
  return pack_impl<unsigned short>(srcs, flat, offsets, (float)scale, like);
}

// dsts[t][i] = float(flat[offsets[t] + i]) over dsts[t]'s flat dense
// storage; a None destination is skipped. Returns the number of kernels
// launched.
int64_t grad_unpack_multi(torch::Tensor flat, std::vector<int64_t> offsets,
                          std::vector<c10::optional<torch::Tensor>> dsts) {
  check_flat(flat, "grad_unpack_multi");
  TORCH_CHECK(dsts.size() == offsets.size(),
              "grad_unpack_multi: offsets and dsts differ in length");
  if (flat.scalar_type() == at::kFloat)
    return unpack_impl<float>(flat, offsets, dsts);
  return unpack_impl<unsigned short>(flat, offsets, dsts);
}
