// Fused NHWC bf16 max-pool forward/backward for gfx950.
//
// Motivation (profiles/kernels_fused_r2.txt): the generic pooling path
// writes an int64 index per output element (8 B each, read again in
// backward), scatters the gradient through shared memory and keeps the
// pool input alive for autograd. Here the forward stores a ONE-BYTE
// window-local argmax (kh*K + kw) and the backward is a gather: every
// input element is written exactly once, so there is no memset of dx,
// there are no atomics and the result is deterministic.
//
// Conventions are bn_relu.hip's: channels-last bf16, C % 8 == 0, one
// lane owns 8 CONSECUTIVE channels (one 16-byte access), 64-bit element
// offsets (VGG16's first pool at bs256 is 822 M elements), threads left
// over when C/8 does not divide the block idle. Pixel counts (N*H*W)
// are 32-bit; the host checks that.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <vector>

typedef __attribute__((ext_vector_type(8))) unsigned short ushort8;

namespace {

__device__ __forceinline__ float pool_bf16_to_f32(unsigned short u) {
  union {
    unsigned int i;
    float f;
  } v;
  v.i = ((unsigned int)u) << 16;
  return v.f;
}

__device__ __forceinline__ unsigned short pool_f32_to_bf16(float f) {
  union {
    float f;
    unsigned int i;
  } v;
  v.f = f;
  // round-to-nearest-even (matches PyTorch's float->bf16 cast)
  unsigned int lsb = (v.i >> 16) & 1;
  v.i += 0x7fffu + lsb;
  return (unsigned short)(v.i >> 16);
}

}  // namespace

#define KS_POOL_BLOCK 256

// --------------------------------------------------------------- forward
// One lane = 8 channels of one output pixel. The K*K loads go to
// CLAMPED (always in-bounds) addresses so they are unconditional and all
// in flight before the first compare; positions that fall into the
// padding are masked out of the scan instead.
// Rule (PyTorch's, row-major over the in-bounds window positions):
//   if (val > maxval || isnan(val)) take it
// starting from maxval = -inf and the first in-bounds position.
template <int K, int S, bool WANT_IDX>
__global__ void max_pool_nhwc_fwd_kernel(const ushort8* __restrict__ x,
                                         ushort8* __restrict__ y,
                                         uint2* __restrict__ idx,
                                         int H, int W, int OH, int OW,
                                         int pad, int M, int CG) {
  const int tid = threadIdx.x;
  const int cg = tid % CG;
  const int roff = tid / CG;
  const int rows_per_blk = KS_POOL_BLOCK / CG;
  // tail threads would alias the next block's pixels: they idle
  if (roff >= rows_per_blk) return;
  const long long row64 = (long long)blockIdx.x * rows_per_blk + roff;
  if (row64 >= M) return;
  const int row = (int)row64;        // output pixel (n, oh, ow)
  const int ow = row % OW;
  const int t = row / OW;
  const int oh = t % OH;
  const int n = t / OH;
  const int h0 = oh * S - pad;
  const int w0 = ow * S - pad;

  ushort8 v[K * K];
  bool ok[K * K];
#pragma unroll
  for (int kh = 0; kh < K; kh++) {
    const int h = h0 + kh;
    const int hc = h < 0 ? 0 : (h >= H ? H - 1 : h);
#pragma unroll
    for (int kw = 0; kw < K; kw++) {
      const int w = w0 + kw;
      const int wc = w < 0 ? 0 : (w >= W ? W - 1 : w);
      ok[kh * K + kw] = (h == hc) && (w == wc);
      const long long pix = ((long long)n * H + hc) * W + wc;
      v[kh * K + kw] = x[pix * CG + cg];
    }
  }

  // first in-bounds position of the window (pad < K: there is one)
  const unsigned int q0 =
      (unsigned int)((h0 < 0 ? -h0 : 0) * K + (w0 < 0 ? -w0 : 0));
  float best[8];
  unsigned int code[8];
  ushort8 o;  // the winner's bf16 bits: the max of bf16 values is exact
#pragma unroll
  for (int j = 0; j < 8; j++) {
    best[j] = -INFINITY;
    code[j] = q0;
    o[j] = 0xff80u;  // -inf
  }
#pragma unroll
  for (int q = 0; q < K * K; q++) {
    if (ok[q]) {
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const float f = pool_bf16_to_f32(v[q][j]);
        if (f > best[j] || f != f) {
          best[j] = f;
          o[j] = v[q][j];
          code[j] = q;
        }
      }
    }
  }

  const long long k = (long long)row * CG + cg;
  y[k] = o;
  if (WANT_IDX) {
    uint2 c;
    c.x = code[0] | (code[1] << 8) | (code[2] << 16) | (code[3] << 24);
    c.y = code[4] | (code[5] << 8) | (code[6] << 16) | (code[7] << 24);
    idx[k] = c;
  }
}

// -------------------------------------------------------------- backward
// One lane = 8 channels of one INPUT pixel (n, h, w). The windows that
// cover it are oh in [ceil((h+pad-K+1)/S), floor((h+pad)/S)] clamped to
// [0, OH) (same for ow): at most NW = ceil(K/S) per axis. They are
// visited in ascending (oh, ow) order; dy is added where the stored code
// equals this pixel's position inside that window. f32 accumulation, one
// RNE rounding, and EVERY input element is written (zero if unselected).
template <int K, int S>
__global__ void max_pool_nhwc_bwd_kernel(const ushort8* __restrict__ dy,
                                         const uint2* __restrict__ idx,
                                         ushort8* __restrict__ dx,
                                         int H, int W, int OH, int OW,
                                         int pad, int M, int CG) {
  constexpr int NW = (K + S - 1) / S;
  const int tid = threadIdx.x;
  const int cg = tid % CG;
  const int roff = tid / CG;
  const int rows_per_blk = KS_POOL_BLOCK / CG;
  if (roff >= rows_per_blk) return;  // see the forward kernel
  const long long row64 = (long long)blockIdx.x * rows_per_blk + roff;
  if (row64 >= M) return;
  const int row = (int)row64;        // input pixel (n, h, w)
  const int w = row % W;
  const int t = row / W;
  const int h = t % H;
  const int n = t / H;

  const int th = h + pad - K + 1;
  const int tw = w + pad - K + 1;
  const int oh_lo = th <= 0 ? 0 : (th + S - 1) / S;
  const int ow_lo = tw <= 0 ? 0 : (tw + S - 1) / S;
  int oh_hi = (h + pad) / S;
  int ow_hi = (w + pad) / S;
  oh_hi = oh_hi < OH ? oh_hi : OH - 1;
  ow_hi = ow_hi < OW ? ow_hi : OW - 1;

  ushort8 g[NW * NW];
  uint2 c[NW * NW];
  bool ok[NW * NW];
  unsigned int want[NW * NW];
#pragma unroll
  for (int a = 0; a < NW; a++) {
    const int oh = oh_lo + a;
    // clamped coordinates keep the load in bounds when the window does
    // not exist (OH >= 1 always)
    const int ohc = oh < OH ? oh : OH - 1;
#pragma unroll
    for (int b = 0; b < NW; b++) {
      const int ow = ow_lo + b;
      const int owc = ow < OW ? ow : OW - 1;
      const int q = a * NW + b;
      ok[q] = oh <= oh_hi && ow <= ow_hi;
      want[q] = (unsigned int)((h + pad - oh * S) * K + (w + pad - ow * S));
      const long long k =
          (((long long)n * OH + ohc) * OW + owc) * CG + cg;
      g[q] = dy[k];
      c[q] = idx[k];
    }
  }

  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; j++) acc[j] = 0.f;
#pragma unroll
  for (int q = 0; q < NW * NW; q++) {
    if (ok[q]) {
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const unsigned int word = j < 4 ? c[q].x : c[q].y;
        const unsigned int code = (word >> (8 * (j & 3))) & 0xffu;
        if (code == want[q]) acc[j] += pool_bf16_to_f32(g[q][j]);
      }
    }
  }
  ushort8 o;
#pragma unroll
  for (int j = 0; j < 8; j++) o[j] = pool_f32_to_bf16(acc[j]);
  dx[(long long)row * CG + cg] = o;
}

// ================================================================== host
namespace {

struct PoolGeom {
  int N, C, H, W, OH, OW, CG;
};

void check_cfg(int64_t k, int64_t s, int64_t p) {
  TORCH_CHECK((k == 3 && s == 2 && p == 1) || (k == 2 && s == 2 && p == 0),
              "max_pool_nhwc: (k, s, p) must be (3, 2, 1) or (2, 2, 0)");
}

PoolGeom pool_geom(int64_t N, int64_t C, int64_t H, int64_t W, int64_t k,
                   int64_t s, int64_t p) {
  TORCH_CHECK(C % 8 == 0 && C >= 8 && C <= KS_POOL_BLOCK * 8,
              "max_pool_nhwc: C must be a multiple of 8 and <= "
              "8*KS_POOL_BLOCK");
  TORCH_CHECK(N >= 1 && H + 2 * p >= k && W + 2 * p >= k,
              "max_pool_nhwc: empty output");
  TORCH_CHECK(N * H * W < (1LL << 31),
              "max_pool_nhwc: N*H*W must fit 32 bits");
  PoolGeom g;
  g.N = (int)N;
  g.C = (int)C;
  g.H = (int)H;
  g.W = (int)W;
  g.OH = (int)((H + 2 * p - k) / s + 1);
  g.OW = (int)((W + 2 * p - k) / s + 1);
  g.CG = g.C / 8;
  return g;
}

unsigned int blocks_for(long long M, int CG) {
  const int rows_per_blk = KS_POOL_BLOCK / CG;
  return (unsigned int)((M + rows_per_blk - 1) / rows_per_blk);
}

}  // namespace

std::vector<torch::Tensor> max_pool_nhwc_fwd(torch::Tensor x, int64_t k,
                                             int64_t s, int64_t p,
                                             bool want_idx) {
  check_cfg(k, s, p);
  TORCH_CHECK(x.is_cuda() && x.dim() == 4, "max_pool_nhwc: 4D GPU tensor");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "max_pool_nhwc: bf16 only");
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast),
              "max_pool_nhwc: channels-last only");
  PoolGeom g = pool_geom(x.size(0), x.size(1), x.size(2), x.size(3), k, s, p);
  auto stream = at::cuda::getCurrentCUDAStream();
  auto y = at::empty({g.N, g.C, g.OH, g.OW},
                     x.options().memory_format(at::MemoryFormat::ChannelsLast));
  torch::Tensor idx;
  if (want_idx)
    idx = at::empty({g.N, g.OH, g.OW, g.C}, x.options().dtype(at::kByte));
  const long long M = (long long)g.N * g.OH * g.OW;
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(blocks_for(M, g.CG)), dim3(KS_POOL_BLOCK),
                       0, stream.stream(),
                       reinterpret_cast<const ushort8*>(x.data_ptr()),
                       reinterpret_cast<ushort8*>(y.data_ptr()),
                       want_idx ? reinterpret_cast<uint2*>(idx.data_ptr())
                                : nullptr,
                       g.H, g.W, g.OH, g.OW, (int)p, (int)M, g.CG);
  };
  if (k == 3)
    want_idx ? launch(max_pool_nhwc_fwd_kernel<3, 2, true>)
             : launch(max_pool_nhwc_fwd_kernel<3, 2, false>);
  else
    want_idx ? launch(max_pool_nhwc_fwd_kernel<2, 2, true>)
             : launch(max_pool_nhwc_fwd_kernel<2, 2, false>);
  if (!want_idx) return {y};
  return {y, idx};
}

torch::Tensor max_pool_nhwc_bwd(torch::Tensor dy, torch::Tensor idx,
                                std::vector<int64_t> input_sizes, int64_t k,
                                int64_t s, int64_t p) {
  check_cfg(k, s, p);
  TORCH_CHECK(input_sizes.size() == 4, "max_pool_nhwc_bwd: 4 input sizes");
  PoolGeom g = pool_geom(input_sizes[0], input_sizes[1], input_sizes[2],
                         input_sizes[3], k, s, p);
  TORCH_CHECK(dy.is_cuda() && dy.dim() == 4 &&
                  dy.scalar_type() == at::kBFloat16 && dy.size(0) == g.N &&
                  dy.size(1) == g.C && dy.size(2) == g.OH &&
                  dy.size(3) == g.OW,
              "max_pool_nhwc_bwd: dy must be bf16 (N, C, OH, OW)");
  TORCH_CHECK(idx.is_cuda() && idx.scalar_type() == at::kByte &&
                  idx.is_contiguous() && idx.dim() == 4 &&
                  idx.size(0) == g.N && idx.size(1) == g.OH &&
                  idx.size(2) == g.OW && idx.size(3) == g.C,
              "max_pool_nhwc_bwd: idx must be uint8 (N, OH, OW, C)");
  if (!dy.is_contiguous(at::MemoryFormat::ChannelsLast))
    dy = dy.contiguous(at::MemoryFormat::ChannelsLast);
  auto stream = at::cuda::getCurrentCUDAStream();
  auto dx = at::empty({g.N, g.C, g.H, g.W},
                      dy.options().memory_format(at::MemoryFormat::ChannelsLast));
  const long long M = (long long)g.N * g.H * g.W;
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(blocks_for(M, g.CG)), dim3(KS_POOL_BLOCK),
                       0, stream.stream(),
                       reinterpret_cast<const ushort8*>(dy.data_ptr()),
                       reinterpret_cast<const uint2*>(idx.data_ptr()),
                       reinterpret_cast<ushort8*>(dx.data_ptr()), g.H, g.W,
                       g.OH, g.OW, (int)p, (int)M, g.CG);
  };
  if (k == 3)
    launch(max_pool_nhwc_bwd_kernel<3, 2>);
  else
    launch(max_pool_nhwc_bwd_kernel<2, 2>);
  return dx;
}
