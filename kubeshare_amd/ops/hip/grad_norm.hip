// Deterministic multi-tensor sums of squares for gfx950: the global
// gradient norm (clipping) and the per-tensor ||g_t||, ||w_t|| (LARS)
// that ops.FusedSGD's update kernel reads from device memory.
//
// Two kernels, no atomics, no host round trip, capturable in a hipGraph:
//
//  stage 1  sumsq_multi_kernel<G>: built like sgd_mom_multi_f32_kernel
//           (ks_ops.hip) and grad_bucket.hip. Pointers, element counts
//           and the block prefix table travel BY VALUE in the kernel
//           arguments; a block binary-searches the table for its tensor,
//           owns one KS_NORM_CHUNK-element chunk of it and writes ONE f32
//           partial with a plain store (two with LARS: the same chunk of
//           the weight).
//  stage 2  norm_finalize_kernel: one block. Waves take tensors
//           round-robin and sum a tensor's partials; wave 0 then sums the
//           tensors and writes norm, clip coefficient and the finite
//           flag (layout: grad_norm.h).
//
// Summation tree. A chunk is a sequence of 8-element groups; thread `tid`
// owns groups tid, tid + 256, ... (8 of them in a full chunk) and keeps
// one accumulator per position in the group, acc[j] = fma(x, x, acc[j]).
// Which elements meet in which accumulator therefore depends on the
// element index alone: the 16-byte vector path, the scalar path of a
// misaligned view and the zero-filled ragged tail add the same numbers in
// the same order, and an f32 tensor holding bf16 values sums to the bits
// of its bf16 twin. Depth of any element's path to the total, in
// sequential f32 roundings:
//   thread   8 fma + 3 (pairwise over the 8 accumulators)        11
//   wave     6 (shuffle tree)   block  3 (4 waves, wave order)     9
//   tensor   ceil(blocks / 64) <= 192 lane-strided + 6 (tree)    198
//   total    ceil(T / 64) <= 16 lane-strided + 6 (tree)           22
// = 240 < 300 for every supported size: T <= KS_NORM_MAX_T tensors of at
// most 64 * 192 chunks (201 M elements) each; beyond that the host code
// raises. All terms are >= 0, so the relative error of a sum is at most
// depth * 2^-24.
//
// A square that overflows f32 (|x| > 1.8e19) makes the total infinite and
// the step count as non-finite.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <vector>

#include "cast_common.h"
#include "grad_norm.h"

#define KS_NORM_THREADS 256
#define KS_NORM_WAVES (KS_NORM_THREADS / 64)
#define KS_NORM_VPT 8  // 8-element groups per thread in a full chunk
#define KS_NORM_CHUNK (KS_NORM_THREADS * KS_NORM_VPT * 8)  // 16384
#define KS_NORM_MAX_TENSORS 110  // per stage-1 launch, as the SGD kernel
#define KS_NORM_MAX_T 1000       // per finalize launch
#define KS_NORM_MAX_TENSOR_BLOCKS (64 * 192)
#define KS_NORM_FIN_THREADS 1024
#define KS_NORM_FIN_WAVES (KS_NORM_FIN_THREADS / 64)

typedef __attribute__((ext_vector_type(8))) unsigned short norm_ushort8;

// G is float, or unsigned short holding bf16 bits
template <typename G>
struct SumsqArgs {
  const G* g[KS_NORM_MAX_TENSORS];
  const float* w[KS_NORM_MAX_TENSORS];  // read only if pw != nullptr
  long long n[KS_NORM_MAX_TENSORS];
  // blk[t] = first block of tensor t; blk[count] = grid size. A tensor
  // without a gradient owns no block (blk[t + 1] == blk[t]).
  int blk[KS_NORM_MAX_TENSORS + 1];
  int count;
  float* pg;  // partial of this launch's block 0
  float* pw;  // the same for the weights; nullptr without LARS
};
static_assert(sizeof(SumsqArgs<float>) <= 4096 &&
                  sizeof(SumsqArgs<unsigned short>) <= 4096,
              "SumsqArgs must fit the 4 KiB kernel-argument segment");

struct NormFinalArgs {
  // off[t] = first partial of tensor t over ALL stage-1 launches;
  // off[count] = number of partials
  int off[KS_NORM_MAX_T + 1];
  float* ws;
  int count;
  int lars;
  int tally;       // add !finite to ws[KS_NORM_WS_COUNT]
  float max_norm;  // <= 0: no clipping, coef = 1
};
static_assert(sizeof(NormFinalArgs) <= 4096,
              "NormFinalArgs must fit the 4 KiB kernel-argument segment");

struct NormF8 {
  float x[8];
};

__device__ __forceinline__ NormF8 norm_load8(const float* p, int k) {
  const float4* p4 = reinterpret_cast<const float4*>(p);
  const float4 lo = p4[2 * k], hi = p4[2 * k + 1];
  return {{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w}};
}
__device__ __forceinline__ NormF8 norm_load8(const unsigned short* p, int k) {
  const norm_ushort8 u = reinterpret_cast<const norm_ushort8*>(p)[k];
  NormF8 f;
#pragma unroll
  for (int j = 0; j < 8; j++) f.x[j] = cast_bf16_to_f32(u[j]);
  return f;
}
__device__ __forceinline__ float norm_load1(const float* p, int i) {
  return p[i];
}
__device__ __forceinline__ float norm_load1(const unsigned short* p, int i) {
  return cast_bf16_to_f32(p[i]);
}

// lane 0 ends with the sum of the wave, by a fixed tree
__device__ __forceinline__ float norm_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// This thread's share of sum(x[i]^2) over one chunk of len elements (see
// the summation tree above).
template <typename G>
__device__ __forceinline__ float norm_chunk_sumsq(const G* __restrict__ x,
                                                  int len, int tid) {
  // the chunk starts a multiple of 16 bytes into the tensor
  const bool vec = ((uintptr_t)x & 15) == 0;
  float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (vec && len == KS_NORM_CHUNK) {
    NormF8 v[KS_NORM_VPT];
#pragma unroll
    for (int u = 0; u < KS_NORM_VPT; u++)
      v[u] = norm_load8(x, tid + u * KS_NORM_THREADS);
#pragma unroll
    for (int u = 0; u < KS_NORM_VPT; u++)
#pragma unroll
      for (int j = 0; j < 8; j++) acc[j] = fmaf(v[u].x[j], v[u].x[j], acc[j]);
  } else {
    for (int k = tid; k * 8 < len; k += KS_NORM_THREADS) {
      const int e = k * 8;
      NormF8 v;
      if (vec && e + 8 <= len) {
        v = norm_load8(x, k);
      } else {
#pragma unroll
        for (int j = 0; j < 8; j++)
          v.x[j] = e + j < len ? norm_load1(x, e + j) : 0.0f;
      }
#pragma unroll
      for (int j = 0; j < 8; j++) acc[j] = fmaf(v.x[j], v.x[j], acc[j]);
    }
  }
  return ((acc[0] + acc[1]) + (acc[2] + acc[3])) +
         ((acc[4] + acc[5]) + (acc[6] + acc[7]));
}

template <typename G>
__global__ void KS_NO_PK_F32 __launch_bounds__(KS_NORM_THREADS)
sumsq_multi_kernel(const SumsqArgs<G> a) {
  __shared__ float s_g[KS_NORM_WAVES], s_w[KS_NORM_WAVES];
  const int b = blockIdx.x;
  // largest t with blk[t] <= b: blk[t + 1] > b then, so tensor t owns
  // block b whether or not its neighbours own any
  int lo = 0, hi = a.count - 1;
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (a.blk[mid] <= b) lo = mid; else hi = mid - 1;
  }
  const long long base = (long long)(b - a.blk[lo]) * KS_NORM_CHUNK;
  const long long rem = a.n[lo] - base;  // > 0 by construction of blk
  const int len = rem < KS_NORM_CHUNK ? (int)rem : KS_NORM_CHUNK;
  const int tid = threadIdx.x;
  const bool lars = a.pw != nullptr;
  float sg = norm_wave_sum(norm_chunk_sumsq(a.g[lo] + base, len, tid));
  float sw = 0.0f;
  if (lars) sw = norm_wave_sum(norm_chunk_sumsq(a.w[lo] + base, len, tid));
  if ((tid & 63) == 0) {
    s_g[tid >> 6] = sg;
    s_w[tid >> 6] = sw;
  }
  __syncthreads();
  if (tid == 0) {
    sg = s_g[0];
    sw = s_w[0];
#pragma unroll
    for (int w = 1; w < KS_NORM_WAVES; w++) {
      sg += s_g[w];
      sw += s_w[w];
    }
    a.pg[b] = sg;
    if (lars) a.pw[b] = sw;
  }
}

__global__ void KS_NO_PK_F32 __launch_bounds__(KS_NORM_FIN_THREADS)
norm_finalize_kernel(const NormFinalArgs a) {
  __shared__ float s_t[KS_NORM_MAX_T];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int T = a.count;
  float* ws = a.ws;
  float* sumsq_g = ws + KS_NORM_WS_HEAD;
  float* sumsq_w = sumsq_g + T;
  float* tnorm = sumsq_w + T;
  const float* pg = tnorm + T;
  const float* pw = pg + a.off[T];
  for (int t = wave; t < T; t += KS_NORM_FIN_WAVES) {
    const int b0 = a.off[t], b1 = a.off[t + 1];
    float sg = 0.0f, sw = 0.0f;
    for (int i = b0 + lane; i < b1; i += 64) sg += pg[i];
    sg = norm_wave_sum(sg);
    if (a.lars) {
      for (int i = b0 + lane; i < b1; i += 64) sw += pw[i];
      sw = norm_wave_sum(sw);
    }
    if (lane == 0) {
      s_t[t] = sg;
      sumsq_g[t] = sg;
      tnorm[t] = sqrtf(sg);
      if (a.lars) sumsq_w[t] = sw;
    }
  }
  __syncthreads();
  if (wave != 0) return;
  float total = 0.0f;
  for (int t = lane; t < T; t += 64) total += s_t[t];
  total = norm_wave_sum(total);
  if (lane != 0) return;
  const float norm = sqrtf(total);
  const bool finite = isfinite(total);
  ws[KS_NORM_WS_NORM] = norm;
  // torch.nn.utils.clip_grad_norm_'s coefficient
  ws[KS_NORM_WS_COEF] =
      a.max_norm > 0.0f ? fminf(1.0f, a.max_norm / (norm + 1e-6f)) : 1.0f;
  ws[KS_NORM_WS_FINITE] = finite ? 1.0f : 0.0f;
  if (a.tally && !finite) {
    int* count = reinterpret_cast<int*>(ws + KS_NORM_WS_COUNT);
    count[0] = count[0] + 1;  // one thread of one block: no atomic
  }
}

namespace {

template <typename G>
int64_t sumsq_launch(const std::vector<c10::optional<torch::Tensor>>& grads,
                     const std::vector<c10::optional<torch::Tensor>>& weights,
                     const NormFinalArgs& f, hipStream_t stream) {
  const bool lars = f.lars != 0;
  float* partials = f.ws + KS_NORM_WS_HEAD + 3 * f.count;
  SumsqArgs<G> a = {};
  int64_t launches = 0;
  int first = 0;  // the tensor in slot 0 of the launch being filled
  a.count = 0;
  a.blk[0] = 0;
  auto flush = [&]() {
    if (a.blk[a.count] > 0) {
      a.pg = partials + f.off[first];
      a.pw = lars ? a.pg + f.off[f.count] : nullptr;
      hipLaunchKernelGGL(sumsq_multi_kernel<G>, dim3(a.blk[a.count]),
                         dim3(KS_NORM_THREADS), 0, stream, a);
      launches++;
    }
    first += a.count;
    a.count = 0;
  };
  for (int t = 0; t < f.count; t++) {
    if (a.count == KS_NORM_MAX_TENSORS) flush();
    const int nb = f.off[t + 1] - f.off[t];
    a.g[a.count] = nb ? static_cast<const G*>((*grads[t]).data_ptr()) : nullptr;
    a.w[a.count] = nb && lars ? (*weights[t]).data_ptr<float>() : nullptr;
    a.n[a.count] = nb ? (*grads[t]).numel() : 0;
    a.blk[a.count + 1] = a.blk[a.count] + nb;
    a.count++;
  }
  flush();
  return launches;
}

}  // namespace

// Stage 1 over grads (f32 or bf16, dense, one dtype; None counts as
// zero) and, if weights is not empty, over the f32 weights of the same
// sizes, then the finalize kernel, into the workspace ws (grad_norm.h;
// >= grad_norm_ws_size elements). max_norm <= 0: no clipping. tally:
// count a non-finite total in ws[3]. Returns the number of launches.
int64_t grad_sumsq_multi(std::vector<c10::optional<torch::Tensor>> grads,
                         std::vector<c10::optional<torch::Tensor>> weights,
                         torch::Tensor ws, double max_norm, bool tally) {
  const char* name = "grad_sumsq_multi";
  auto stream = at::cuda::getCurrentCUDAStream();
  TORCH_CHECK(grads.size() <= KS_NORM_MAX_T, name, ": at most ",
              KS_NORM_MAX_T, " tensors, got ", grads.size());
  const bool lars = !weights.empty();
  TORCH_CHECK(!lars || weights.size() == grads.size(), name,
              ": grads and weights differ in length");
  TORCH_CHECK(ws.is_cuda() && ws.dim() == 1 && ws.is_contiguous() &&
                  ws.scalar_type() == at::kFloat &&
                  ws.get_device() == stream.device_index(),
              name, ": the workspace is a contiguous 1-D f32 tensor on the "
              "current device");
  NormFinalArgs f = {};
  f.ws = ws.data_ptr<float>();
  f.count = (int)grads.size();
  f.lars = lars;
  f.tally = tally;
  f.max_norm = (float)max_norm;
  f.off[0] = 0;
  auto gtype = at::kFloat;
  bool typed = false;
  long long total = 0;
  for (int t = 0; t < f.count; t++) {
    long long nb = 0;
    if (grads[t].has_value() && grads[t]->defined() &&
        grads[t]->numel() > 0) {
      const torch::Tensor& g = *grads[t];
      if (!typed) gtype = g.scalar_type();
      typed = true;
      TORCH_CHECK(gtype == at::kFloat || gtype == at::kBFloat16, name,
                  ": f32 or bf16 tensors expected");
      TORCH_CHECK(g.is_cuda() && g.scalar_type() == gtype &&
                      g.is_non_overlapping_and_dense() &&
                      g.get_device() == stream.device_index(),
                  name, ": dense tensors of one dtype on the current device "
                  "expected");
      nb = (g.numel() + KS_NORM_CHUNK - 1) / KS_NORM_CHUNK;
      TORCH_CHECK(nb <= KS_NORM_MAX_TENSOR_BLOCKS, name, ": a tensor of ",
                  g.numel(), " elements exceeds the ",
                  (long long)KS_NORM_MAX_TENSOR_BLOCKS * KS_NORM_CHUNK,
                  " the summation-depth bound allows");
      if (lars) {
        TORCH_CHECK(weights[t].has_value() && weights[t]->defined(), name,
                    ": a gradient without its weight");
        const torch::Tensor& w = *weights[t];
        TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kFloat &&
                        w.is_non_overlapping_and_dense() &&
                        w.numel() == g.numel() &&
                        w.get_device() == g.get_device(),
                    name, ": dense f32 weights of the gradients' sizes "
                    "expected");
      }
    }
    total += nb;
    TORCH_CHECK(total < (1LL << 30), name, ": too many elements");
    f.off[t + 1] = (int)total;
  }
  TORCH_CHECK(ws.numel() >= KS_NORM_WS_HEAD + 3LL * f.count +
                                (lars ? 2 : 1) * total,
              name, ": workspace of ", ws.numel(), " elements is too small");
  int64_t launches =
      gtype == at::kFloat
          ? sumsq_launch<float>(grads, weights, f, stream.stream())
          : sumsq_launch<unsigned short>(grads, weights, f, stream.stream());
  hipLaunchKernelGGL(norm_finalize_kernel, dim3(1),
                     dim3(KS_NORM_FIN_THREADS), 0, stream.stream(), f);
  return launches + 1;
}

// Elements a workspace needs for tensors of these element counts.
int64_t grad_norm_ws_size(std::vector<int64_t> numels, bool lars) {
  int64_t blocks = 0;
  for (int64_t n : numels) blocks += (n + KS_NORM_CHUNK - 1) / KS_NORM_CHUNK;
  return KS_NORM_WS_HEAD + 3 * (int64_t)numels.size() +
         (lars ? 2 : 1) * blocks;
}
