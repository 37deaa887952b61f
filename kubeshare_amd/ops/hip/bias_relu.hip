// Fused NHWC bf16 bias + ReLU (+ max-pool) for gfx950: the conv layers
// of BN-free networks (torchvision's plain VGG16: thirteen
// conv(+bias) -> ReLU pairs, five of them followed by a 2x2 max-pool).
//
// The stock eager path runs, per conv layer, an in-place add of the
// bias, an in-place ReLU and where there is one the pool; backward, the
// pool backward writes a full-resolution gradient that
// threshold_backward re-reads, and the bias gradient is a separate sum
// over that result. Here:
//
//   bias_relu_fwd_kernel       y = bf16(relu(f32(x) + b[c])): one read
//                              of x, one write of y. b is f32 and is NOT
//                              rounded to bf16 first (autocast's modules
//                              do round it).
//   bias_relu_bwd_kernel       dx = y > 0 ? dy : 0 (the bits of dy, or
//                              zero) and db[c] = sum(dx) in one pass:
//                              per-lane f32 accumulators, an LDS tree per
//                              block, part[blocks][C], then one launch of
//                              bn_relu.hip's coalesced reduce.
//   bias_relu_pool_fwd_kernel  one lane owns 8 channels of one OUTPUT
//                              pixel; every in-bounds window value goes
//                              through the expression above (rounded to
//                              bf16 BEFORE comparing) and then through
//                              pool.hip's scan. The full-resolution
//                              activation is never written.
//   bias_relu_pool_bwd_kernel  one lane owns 8 channels of one INPUT
//                              pixel, gathers as max_pool_nhwc_bwd_kernel
//                              does and masks with the POOLED y.
//
// Why the pool backward needs neither x nor the full-resolution y:
// v -> bf16(relu(v + b)) is monotone non-decreasing per channel, so the
// pooled output is the value of the element the code points at. That
// element's ReLU mask (y_full > 0) is therefore (y_pooled > 0) of every
// window that selected it: the pooled y and the one-byte codes say all
// the backward has to know.
//
// Layout, row walk (NhwcRows) and block partials are nhwc_common.h's,
// the window scan, the gather (PoolGather<.., WITH_Y>) and the pool
// geometry pool_window.h's; arithmetic is f32.
// No atomics: every result is a fixed-order sum.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <vector>

#include "bn_common.h"
#include "pool_window.h"

// Rows loaded per sub-batch of a KS_BN_UNROLL group in the pooled
// backward (see bn_pool.hip): a (3, 2, 1) row carries 4 gradient
// vectors, 4 pooled-y vectors and 4 code words.
#define KS_BR_U_321 1
#define KS_BR_U_220 2

// The forward expression, in one place: the pooled kernel must produce a
// value the unpooled kernel would have written.
__device__ __forceinline__ unsigned short bias_relu_bf16(unsigned short x,
                                                         float b) {
  return bn_relu_bf16(bf16_to_f32(x) + b);
}

// --------------------------------------------------------------- forward
__global__ void __launch_bounds__(KS_BN_BLOCK)
bias_relu_fwd_kernel(const ushort8* __restrict__ x, ushort8* __restrict__ y,
                     const float* __restrict__ bias, long long M, int CG) {
  const NhwcRows<KS_BN_BLOCK> rows(CG);
  const int cg = rows.cg;
  const long long stride = rows.stride;
  float8 b;
#pragma unroll
  for (int j = 0; j < 8; j++) b[j] = bias[cg * 8 + j];
  auto one = [&](const ushort8& v) {
    ushort8 o;
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = bias_relu_bf16(v[j], b[j]);
    return o;
  };
  long long row = rows.first(M);
  for (; row + (KS_BN_UNROLL - 1) * stride < M;
       row += KS_BN_UNROLL * stride) {
    ushort8 v[KS_BN_UNROLL];
    long long k[KS_BN_UNROLL];
#pragma unroll
    for (int u = 0; u < KS_BN_UNROLL; u++) {
      k[u] = (row + u * stride) * CG + cg;
      v[u] = x[k[u]];
    }
#pragma unroll
    for (int u = 0; u < KS_BN_UNROLL; u++) y[k[u]] = one(v[u]);
  }
  for (; row < M; row += stride) {
    const long long k = row * CG + cg;
    const ushort8 v = x[k];
    y[k] = one(v);
  }
}

// -------------------------------------------------------------- backward
// dx = y > 0 ? dy : 0, db partials: part[b*C + c].
__global__ void __launch_bounds__(KS_BN_BLOCK)
bias_relu_bwd_kernel(const ushort8* __restrict__ dy,
                     const ushort8* __restrict__ y, ushort8* __restrict__ dx,
                     float* __restrict__ part, long long M, int CG) {
  __shared__ float s_red[KS_BN_BLOCK * 8];
  const NhwcRows<KS_BN_BLOCK> rows(CG);
  const int cg = rows.cg;
  const long long stride = rows.stride;
  float8 adb = {0, 0, 0, 0, 0, 0, 0, 0};
  auto one = [&](const ushort8& gv, const ushort8& yv) {
    ushort8 o;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      o[j] = bf16_to_f32(yv[j]) > 0.f ? gv[j] : (unsigned short)0;
      adb[j] += bf16_to_f32(o[j]);
    }
    return o;
  };
  long long row = rows.first(M);
  for (; row + (KS_BN_UNROLL - 1) * stride < M;
       row += KS_BN_UNROLL * stride) {
    ushort8 gv[KS_BN_UNROLL], yv[KS_BN_UNROLL];
    long long k[KS_BN_UNROLL];
#pragma unroll
    for (int u = 0; u < KS_BN_UNROLL; u++) {
      k[u] = (row + u * stride) * CG + cg;
      gv[u] = dy[k[u]];
      yv[u] = y[k[u]];
    }
#pragma unroll
    for (int u = 0; u < KS_BN_UNROLL; u++) dx[k[u]] = one(gv[u], yv[u]);
  }
  for (; row < M; row += stride) {
    const long long k = row * CG + cg;
    const ushort8 gv = dy[k], yv = y[k];
    dx[k] = one(gv, yv);
  }
  nhwc_block_partials<KS_BN_BLOCK>(s_red, adb, part, CG);
}

// -------------------------------------------------------- pooled forward
// max_pool_nhwc_fwd_kernel with the bias + ReLU applied to every loaded
// value. Rule (pool.hip's): start from -inf at the first in-bounds
// position, take a value if val > best || isnan(val), row-major.
template <int K, int S, bool WANT_IDX>
__global__ void __launch_bounds__(KS_POOL_BLOCK)
bias_relu_pool_fwd_kernel(const ushort8* __restrict__ x,
                          ushort8* __restrict__ y, uint2* __restrict__ idx,
                          const float* __restrict__ bias, int H, int W,
                          int OH, int OW, int pad, int M, int CG) {
  int cg, row;  // output pixel (n, oh, ow)
  if (!nhwc_one_row<KS_POOL_BLOCK>(M, CG, cg, row)) return;
  PoolWindow<K, S> win;
  win.load(x, row, H, W, OH, OW, pad, CG, cg);
  float8 b;
#pragma unroll
  for (int j = 0; j < 8; j++) b[j] = bias[cg * 8 + j];
  // every value as bias_relu_fwd_kernel would have stored it
  unsigned int code[8];
  const ushort8 o = win.scan(
      [&](unsigned short v, int j) { return bias_relu_bf16(v, b[j]); }, code);
  const long long k = (long long)row * CG + cg;
  y[k] = o;
  if (WANT_IDX) idx[k] = pool_pack_codes(code);
}

// ------------------------------------------------------- pooled backward
// PoolGather<K, S, true> (pool_window.h): max_pool_nhwc_bwd_kernel's
// gather plus the pooled y of each covering window.
// Rows are INPUT pixels in the grid-stride structure of
// bias_relu_bwd_kernel. db accumulates the dx this lane writes (the
// rounded sum: with the (3, 2, 1) windows overlapping, a pixel can
// collect up to four dy), so db is the sum of the returned dx as it is
// for the unpooled op; every selected, unmasked dy enters exactly once,
// at the lane that owns the selected pixel.
template <int K, int S, int U>
__global__ void __launch_bounds__(KS_BN_BLOCK)
bias_relu_pool_bwd_kernel(const ushort8* __restrict__ dy,
                          const uint2* __restrict__ idx,
                          const ushort8* __restrict__ y,
                          ushort8* __restrict__ dx, float* __restrict__ part,
                          int H, int W, int OH, int OW, int pad, long long M,
                          int CG) {
  static_assert(KS_BN_UNROLL % U == 0, "sub-batches must tile a group");
  __shared__ float s_red[KS_BN_BLOCK * 8];
  const NhwcRows<KS_BN_BLOCK> rows(CG);
  const int cg = rows.cg;
  const long long stride = rows.stride;
  float8 adb = {0, 0, 0, 0, 0, 0, 0, 0};
  auto one = [&](const PoolGather<K, S, true>& pg) {
    ushort8 o;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      o[j] = pg.grad_bits(j);
      adb[j] += bf16_to_f32(o[j]);
    }
    return o;
  };
  long long row = rows.first(M);
  for (; row + (KS_BN_UNROLL - 1) * stride < M;
       row += KS_BN_UNROLL * stride) {
    // a real loop: unrolled, the next sub-batch's loads are hoisted over
    // this one's arithmetic and the registers run out
#pragma unroll 1
    for (int h = 0; h < KS_BN_UNROLL; h += U) {
      long long k[U];
      PoolGather<K, S, true> pg[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const long long r = row + (h + u) * stride;
        k[u] = r * CG + cg;
        pg[u].load(dy, idx, y, (int)r, H, W, OH, OW, pad, CG, cg);
      }
#pragma unroll
      for (int u = 0; u < U; u++) dx[k[u]] = one(pg[u]);
    }
  }
  for (; row < M; row += stride) {
    PoolGather<K, S, true> pg;
    pg.load(dy, idx, y, (int)row, H, W, OH, OW, pad, CG, cg);
    dx[row * CG + cg] = one(pg);
  }
  nhwc_block_partials<KS_BN_BLOCK>(s_red, adb, part, CG);
}

// ================================================================== host
namespace {

// x-shaped tensor of either op: 4-D bf16 channels-last on the GPU,
// C % 8 == 0, 8 <= C <= 2048, at least one pixel, N*H*W < 2**31
BnGeom geom_of(const torch::Tensor& x, const char* what) {
  TORCH_CHECK(x.is_cuda(), what, ": GPU tensor expected");
  BnGeom g = bn_geom_of(x);  // dim, dtype, layout, C % 8
  TORCH_CHECK(g.C >= 8 && g.C <= KS_POOL_BLOCK * 8, what,
              ": C must be a multiple of 8 in [8, 2048]");
  TORCH_CHECK(g.M >= 1, what, ": empty tensor");
  TORCH_CHECK(g.M < (1LL << 31), what, ": N*H*W must fit 32 bits");
  return g;
}

void check_bias(const BnGeom& g, const torch::Tensor& bias,
                const char* what) {
  TORCH_CHECK(bias.is_cuda() && bias.scalar_type() == at::kFloat &&
                  bias.is_contiguous() && bias.numel() == g.C,
              what, ": bias must be a contiguous f32 GPU tensor of C "
              "elements");
}

// block partials -> db (C) f32
torch::Tensor reduce_db(const torch::Tensor& part, const BnGeom& g,
                        hipStream_t stream) {
  auto db = at::empty({g.C}, part.options());
  bn_launch_reduce_one(part.data_ptr<float>(), g.stat_blocks, g.C,
                       db.data_ptr<float>(), stream);
  return db;
}

}  // namespace

torch::Tensor bias_relu_fwd(torch::Tensor x, torch::Tensor bias) {
  BnGeom g = geom_of(x, "bias_relu_fwd");
  check_bias(g, bias, "bias_relu_fwd");
  auto stream = at::cuda::getCurrentCUDAStream();
  auto y = at::empty_like(x);
  hipLaunchKernelGGL(bias_relu_fwd_kernel, dim3(g.blocks), dim3(KS_BN_BLOCK),
                     0, stream.stream(),
                     nhwc_cptr(x),
                     nhwc_mptr(y),
                     bias.data_ptr<float>(), g.M, g.CG);
  return y;
}

// Returns {dx, db}.
std::vector<torch::Tensor> bias_relu_bwd(torch::Tensor dy, torch::Tensor y) {
  BnGeom g = geom_of(y, "bias_relu_bwd");
  TORCH_CHECK(dy.is_cuda() && dy.scalar_type() == at::kBFloat16 &&
                  dy.sizes() == y.sizes(),
              "bias_relu_bwd: dy must be bf16 of y's shape");
  if (!dy.is_contiguous(at::MemoryFormat::ChannelsLast))
    dy = dy.contiguous(at::MemoryFormat::ChannelsLast);
  auto stream = at::cuda::getCurrentCUDAStream();
  auto dx = at::empty_like(y);
  auto part = at::empty({(long long)g.stat_blocks * g.C},
                        y.options().dtype(at::kFloat));
  hipLaunchKernelGGL(bias_relu_bwd_kernel, dim3(g.stat_blocks),
                     dim3(KS_BN_BLOCK), 0, stream.stream(),
                     nhwc_cptr(dy),
                     nhwc_cptr(y),
                     nhwc_mptr(dx),
                     part.data_ptr<float>(), g.M, g.CG);
  return {dx, reduce_db(part, g, stream.stream())};
}

// Returns {y} or, with want_idx, {y, idx}: y (N, C, OH, OW) bf16
// channels-last, idx (N, OH, OW, C) uint8 window codes.
std::vector<torch::Tensor> bias_relu_pool_fwd(torch::Tensor x,
                                              torch::Tensor bias, int64_t k,
                                              int64_t s, int64_t p,
                                              bool want_idx) {
  pool_check_cfg("bias_relu_pool", k, s, p);
  BnGeom g = geom_of(x, "bias_relu_pool_fwd");
  check_bias(g, bias, "bias_relu_pool_fwd");
  const PoolGeom o = pool_geom("bias_relu_pool", x.size(0), g.C, x.size(2),
                               x.size(3), k, s, p);
  const int N = o.N, H = o.H, W = o.W;
  auto stream = at::cuda::getCurrentCUDAStream();
  auto y = at::empty({N, g.C, o.OH, o.OW},
                     x.options().memory_format(at::MemoryFormat::ChannelsLast));
  torch::Tensor idx;
  if (want_idx)
    idx = at::empty({N, o.OH, o.OW, g.C}, x.options().dtype(at::kByte));
  const long long MO = o.MO;  // <= N*H*W < 2**31
  const unsigned int blocks = pool_blocks_for(MO, g.CG);
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(KS_POOL_BLOCK), 0,
                       stream.stream(),
                       nhwc_cptr(x),
                       nhwc_mptr(y),
                       want_idx ? reinterpret_cast<uint2*>(idx.data_ptr())
                                : nullptr,
                       bias.data_ptr<float>(), H, W, o.OH, o.OW, (int)p,
                       (int)MO, g.CG);
  };
  if (k == 3)
    want_idx ? launch(bias_relu_pool_fwd_kernel<3, 2, true>)
             : launch(bias_relu_pool_fwd_kernel<3, 2, false>);
  else
    want_idx ? launch(bias_relu_pool_fwd_kernel<2, 2, true>)
             : launch(bias_relu_pool_fwd_kernel<2, 2, false>);
  if (!want_idx) return {y};
  return {y, idx};
}

// Returns {dx, db}; reads only dy, the codes and the pooled y.
std::vector<torch::Tensor> bias_relu_pool_bwd(
    torch::Tensor dy, torch::Tensor idx, torch::Tensor y,
    std::vector<int64_t> input_sizes, int64_t k, int64_t s, int64_t p) {
  pool_check_cfg("bias_relu_pool", k, s, p);
  TORCH_CHECK(input_sizes.size() == 4, "bias_relu_pool_bwd: 4 input sizes");
  TORCH_CHECK(input_sizes[0] >= 1 && input_sizes[1] >= 8 &&
                  input_sizes[2] >= 1 && input_sizes[3] >= 1,
              "bias_relu_pool_bwd: empty input");
  TORCH_CHECK(y.is_cuda() && y.dim() == 4 &&
                  y.scalar_type() == at::kBFloat16 &&
                  y.is_contiguous(at::MemoryFormat::ChannelsLast),
              "bias_relu_pool_bwd: y must be a bf16 channels-last GPU "
              "tensor");
  auto dx = at::empty(input_sizes,
                      y.options().memory_format(at::MemoryFormat::ChannelsLast));
  BnGeom g = geom_of(dx, "bias_relu_pool_bwd");
  const PoolGeom o = pool_geom("bias_relu_pool", input_sizes[0], g.C,
                               input_sizes[2], input_sizes[3], k, s, p);
  const int N = o.N, H = o.H, W = o.W;
  TORCH_CHECK(y.size(0) == N && y.size(1) == g.C && y.size(2) == o.OH &&
                  y.size(3) == o.OW,
              "bias_relu_pool_bwd: y must be (N, C, OH, OW)");
  TORCH_CHECK(dy.is_cuda() && dy.scalar_type() == at::kBFloat16 &&
                  dy.sizes() == y.sizes(),
              "bias_relu_pool_bwd: dy must be bf16 (N, C, OH, OW)");
  TORCH_CHECK(idx.is_cuda() && idx.scalar_type() == at::kByte &&
                  idx.is_contiguous() && idx.dim() == 4 &&
                  idx.size(0) == N && idx.size(1) == o.OH &&
                  idx.size(2) == o.OW && idx.size(3) == g.C,
              "bias_relu_pool_bwd: idx must be uint8 (N, OH, OW, C)");
  if (!dy.is_contiguous(at::MemoryFormat::ChannelsLast))
    dy = dy.contiguous(at::MemoryFormat::ChannelsLast);
  auto stream = at::cuda::getCurrentCUDAStream();
  auto part = at::empty({(long long)g.stat_blocks * g.C},
                        y.options().dtype(at::kFloat));
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(g.stat_blocks), dim3(KS_BN_BLOCK), 0,
                       stream.stream(),
                       nhwc_cptr(dy),
                       reinterpret_cast<const uint2*>(idx.data_ptr()),
                       nhwc_cptr(y),
                       nhwc_mptr(dx),
                       part.data_ptr<float>(), H, W, o.OH, o.OW, (int)p, g.M,
                       g.CG);
  };
  if (k == 3)
    launch(bias_relu_pool_bwd_kernel<3, 2, KS_BR_U_321>);
  else
    launch(bias_relu_pool_bwd_kernel<2, 2, KS_BR_U_220>);
  return {dx, reduce_db(part, g, stream.stream())};
}
