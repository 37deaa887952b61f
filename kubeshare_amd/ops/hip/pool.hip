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
// The window scan, the gather and the geometry checks are pool_window.h's
// (shared with bn_pool.hip and bias_relu.hip; the checks are defined
// here); layout conventions and the one-row prologue are nhwc_common.h's.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <vector>

#include "pool_window.h"

// --------------------------------------------------------------- forward
// One lane = 8 channels of one output pixel: PoolWindow's loads and scan
// over the values themselves.
template <int K, int S, bool WANT_IDX>
__global__ void max_pool_nhwc_fwd_kernel(const ushort8* __restrict__ x,
                                         ushort8* __restrict__ y,
                                         uint2* __restrict__ idx,
                                         int H, int W, int OH, int OW,
                                         int pad, int M, int CG) {
  int cg, row;  // output pixel (n, oh, ow)
  if (!nhwc_one_row<KS_POOL_BLOCK>(M, CG, cg, row)) return;
  PoolWindow<K, S> win;
  win.load(x, row, H, W, OH, OW, pad, CG, cg);
  unsigned int code[8];
  const ushort8 o = win.scan([](unsigned short v, int) { return v; }, code);
  const long long k = (long long)row * CG + cg;
  y[k] = o;
  if (WANT_IDX) idx[k] = pool_pack_codes(code);
}

// -------------------------------------------------------------- backward
// One lane = 8 channels of one INPUT pixel (n, h, w): PoolGather's loads
// and sum; EVERY input element is written (zero if unselected).
template <int K, int S>
__global__ void max_pool_nhwc_bwd_kernel(const ushort8* __restrict__ dy,
                                         const uint2* __restrict__ idx,
                                         ushort8* __restrict__ dx,
                                         int H, int W, int OH, int OW,
                                         int pad, int M, int CG) {
  int cg, row;  // input pixel (n, h, w)
  if (!nhwc_one_row<KS_POOL_BLOCK>(M, CG, cg, row)) return;
  PoolGather<K, S> pg;
  pg.load(dy, idx, nullptr, row, H, W, OH, OW, pad, CG, cg);
  ushort8 o;
#pragma unroll
  for (int j = 0; j < 8; j++) o[j] = pg.grad_bits(j);
  dx[(long long)row * CG + cg] = o;
}

// ================================================================== host
void pool_check_cfg(const char* op, int64_t k, int64_t s, int64_t p) {
  TORCH_CHECK((k == 3 && s == 2 && p == 1) || (k == 2 && s == 2 && p == 0),
              op, ": (k, s, p) must be (3, 2, 1) or (2, 2, 0)");
}

PoolGeom pool_geom(const char* op, int64_t N, int64_t C, int64_t H, int64_t W,
                   int64_t k, int64_t s, int64_t p) {
  TORCH_CHECK(C % 8 == 0 && C >= 8 && C <= KS_POOL_BLOCK * 8, op,
              ": C must be a multiple of 8 in [8, 2048]");
  TORCH_CHECK(N >= 1 && H + 2 * p >= k && W + 2 * p >= k, op,
              ": empty output");
  TORCH_CHECK(N * H * W < (1LL << 31), op, ": N*H*W must fit 32 bits");
  PoolGeom g;
  g.N = (int)N;
  g.C = (int)C;
  g.H = (int)H;
  g.W = (int)W;
  g.OH = (int)((H + 2 * p - k) / s + 1);
  g.OW = (int)((W + 2 * p - k) / s + 1);
  g.CG = g.C / 8;
  g.pad = (int)p;
  g.MO = (long long)g.N * g.OH * g.OW;
  return g;
}

std::vector<torch::Tensor> max_pool_nhwc_fwd(torch::Tensor x, int64_t k,
                                             int64_t s, int64_t p,
                                             bool want_idx) {
  pool_check_cfg("max_pool_nhwc", k, s, p);
  TORCH_CHECK(x.is_cuda() && x.dim() == 4, "max_pool_nhwc: 4D GPU tensor");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "max_pool_nhwc: bf16 only");
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast),
              "max_pool_nhwc: channels-last only");
  PoolGeom g = pool_geom("max_pool_nhwc", x.size(0), x.size(1), x.size(2),
                         x.size(3), k, s, p);
  auto stream = at::cuda::getCurrentCUDAStream();
  auto y = at::empty({g.N, g.C, g.OH, g.OW},
                     x.options().memory_format(at::MemoryFormat::ChannelsLast));
  torch::Tensor idx;
  if (want_idx)
    idx = at::empty({g.N, g.OH, g.OW, g.C}, x.options().dtype(at::kByte));
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(pool_blocks_for(g.MO, g.CG)),
                       dim3(KS_POOL_BLOCK), 0, stream.stream(), nhwc_cptr(x),
                       nhwc_mptr(y),
                       want_idx ? reinterpret_cast<uint2*>(idx.data_ptr())
                                : nullptr,
                       g.H, g.W, g.OH, g.OW, g.pad, (int)g.MO, g.CG);
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
  pool_check_cfg("max_pool_nhwc", k, s, p);
  TORCH_CHECK(input_sizes.size() == 4, "max_pool_nhwc_bwd: 4 input sizes");
  PoolGeom g = pool_geom("max_pool_nhwc", input_sizes[0], input_sizes[1],
                         input_sizes[2], input_sizes[3], k, s, p);
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
    hipLaunchKernelGGL(kern, dim3(pool_blocks_for(M, g.CG)),
                       dim3(KS_POOL_BLOCK), 0, stream.stream(), nhwc_cptr(dy),
                       reinterpret_cast<const uint2*>(idx.data_ptr()),
                       nhwc_mptr(dx), g.H, g.W, g.OH, g.OW, g.pad, (int)M,
                       g.CG);
  };
  if (k == 3)
    launch(max_pool_nhwc_bwd_kernel<3, 2>);
  else
    launch(max_pool_nhwc_bwd_kernel<2, 2>);
  return dx;
}
