// Fused NHWC bf16 BatchNorm + ReLU + max-pool for gfx950: the ResNet
// stem and VGG16's five pools, where nothing but the pool ever reads
// the BN output.
//
// The composition ops.max_pool_nhwc(ops.bn_relu(x, bn)) writes the
// full-resolution activation y, reads it straight back, keeps it alive
// for autograd, and in backward writes a full-resolution pool gradient
// that the two BN backward kernels each read back. Here y is never
// allocated, in either direction:
//
//   forward   bn_stats -> bn_reduce_tile<FINALIZE>     (bn_relu.hip, the
//             very launches of bn_relu_fwd_train, through
//             bn_launch_fwd_stats) -> bn_pool_fwd_kernel<K, S, WANT_IDX>
//   eval      bn_fold_eval -> bn_pool_fwd_kernel<K, S, false>
//   backward  bn_pool_bwd_stats_kernel<K, S> -> bn_reduce_tile
//             -> bn_pool_bwd_apply_kernel<K, S>
//
// Kernel inventory:
//  - bn_pool_fwd_kernel: one lane owns 8 channels of one OUTPUT pixel.
//    K*K unconditional loads of x at clamped addresses (as in
//    max_pool_nhwc_fwd_kernel); every loaded value goes through
//    bn_apply_relu_kernel<false, true>'s expression (bn_affine,
//    bn_relu_bf16: rounded to bf16 BEFORE comparing) and then through
//    pool.hip's scan rule. Pooling x first and applying the affine map
//    afterwards would be wrong for channels whose folded scale is
//    negative or zero. The (3, 2, 1) configuration reads each input row
//    about 2.25 times, from cache after the first.
//  - bn_pool_bwd_stats_kernel: rows are INPUT pixels in the grid-stride
//    structure (and launch geometry) of bn_bwd_stats_noy_kernel<true>.
//    Per row the pool gradient is formed in registers exactly as
//    max_pool_nhwc_bwd_kernel forms it (covering windows in ascending
//    (oh, ow) order, f32 sum where the stored code matches, one RNE
//    rounding to bf16), then the recomputed ReLU mask is applied and
//    dbias / dscale go to block partials. Same rows per lane in the same
//    order as the composition: dbias (pure adds) comes out bit-equal.
//  - bn_pool_bwd_apply_kernel: same gather and mask, then
//    dx = w*invstd*(g - dbias/M - xhat*dscale/M), written once.
//
// Rows advance in groups of KS_BN_UNROLL; a group is loaded U rows at a
// time (sub-batches in a real loop, as bn_bwd_stats_kernel's WITH_DY2
// variant does): a (3, 2, 1) row carries 4 gradient vectors, 4 code
// words and x, and four such rows do not fit in registers.
//
// Layout, row walk (NhwcRows) and block partials are nhwc_common.h's,
// the window scan, the gather (PoolGather) and the pool geometry
// pool_window.h's. Every floating-point
// expression whose contraction could differ between instantiations is
// written with explicit fmaf or under contract(off).
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <type_traits>
#include <vector>

#include "bn_common.h"
#include "pool_window.h"

// Rows loaded per sub-batch of a KS_BN_UNROLL group in the backward.
// A 512-thread block is two waves per SIMD, so a second block per CU
// needs 4 waves/SIMD, i.e. at most 128 VGPRs. From
// -Rpass-analysis=kernel-resource-usage (stats / apply kernel, scratch
// 0 everywhere): (3, 2, 1) U=2 134 / 136 VGPRs (3 waves/SIMD: one block
// per CU), U=1 100 / 99 (4 waves/SIMD) with 9 loads in flight per lane;
// (2, 2, 0) U=4 127 / 132 (apply at 3 waves/SIMD), U=2 90 / 91 (5).
#define KS_BNP_U_321 1
#define KS_BNP_U_220 2

// --------------------------------------------------------------- forward
template <int K, int S, bool WANT_IDX>
__global__ void __launch_bounds__(KS_POOL_BLOCK)
bn_pool_fwd_kernel(const ushort8* __restrict__ x, ushort8* __restrict__ y,
                   uint2* __restrict__ idx, const float* __restrict__ scale,
                   const float* __restrict__ biasf, int H, int W, int OH,
                   int OW, int pad, int M, int CG) {
  int cg, row;  // output pixel (n, oh, ow)
  if (!nhwc_one_row<KS_POOL_BLOCK>(M, CG, cg, row)) return;
  PoolWindow<K, S> win;
  win.load(x, row, H, W, OH, OW, pad, CG, cg);
  float8 s, b;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    s[j] = scale[cg * 8 + j];
    b[j] = biasf[cg * 8 + j];
  }
  // every value as bn_apply_relu_kernel<false, true> would have stored it
  unsigned int code[8];
  const ushort8 o = win.scan(
      [&](unsigned short v, int j) {
        return bn_relu_bf16(bn_affine(bf16_to_f32(v), s[j], b[j]));
      },
      code);
  const long long k = (long long)row * CG + cg;
  y[k] = o;
  if (WANT_IDX) idx[k] = pool_pack_codes(code);
}

// -------------------------------------------------------------- backward
// (the gather, PoolGather<K, S>, is pool_window.h's)

// ReLU mask recomputed from x and the folded constants, the expression
// of bn_bwd_stats_noy_kernel: y != 0 <=> bf16(relu(fma(x, s', b'))) != 0
__device__ __forceinline__ bool bn_pool_relu_on(float xf, float sc,
                                                float bf) {
  const float f = fmaf(xf, sc, bf);
  return f32_to_bf16(f > 0.f ? f : 0.f) != 0;
}

// (bn_pool_xhat and bn_pool_dx, shared with bn_join.hip, are in
// bn_common.h)

// folded scale' = w*invstd and bias' = b - mean*scale' as
// bn_finalize_channel computes them (rounded product, then one FMA)
__device__ __forceinline__ float bn_pool_fold_scale(float w, float is) {
  return w * is;
}

__device__ __forceinline__ float bn_pool_fold_bias(float b, float mu,
                                                   float sc) {
  return fmaf(-mu, sc, b);
}

template <int K, int S, int U>
__global__ void __launch_bounds__(KS_BN_BLOCK)
bn_pool_bwd_stats_kernel(const ushort8* __restrict__ x,
                         const ushort8* __restrict__ dy,
                         const uint2* __restrict__ idx,
                         const float* __restrict__ mean,
                         const float* __restrict__ invstd,
                         const float* __restrict__ weight,
                         const float* __restrict__ bias,
                         float* __restrict__ part, int H, int W, int OH,
                         int OW, int pad, long long M, int CG) {
  static_assert(KS_BN_UNROLL % U == 0, "sub-batches must tile a group");
  __shared__ float s_red[KS_BN_BLOCK * 8];
  const NhwcRows<KS_BN_BLOCK> rows(CG);
  const int cg = rows.cg;
  const long long stride = rows.stride;
  float8 mu, is, sc, bf;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int c = cg * 8 + j;
    mu[j] = mean[c];
    is[j] = invstd[c];
    sc[j] = bn_pool_fold_scale(weight[c], is[j]);
    bf[j] = bn_pool_fold_bias(bias[c], mu[j], sc[j]);
  }
  float8 adb = {0, 0, 0, 0, 0, 0, 0, 0};
  float8 ads = {0, 0, 0, 0, 0, 0, 0, 0};
  // one row; `grouped` (std::true_type inside a whole group of four
  // rows) selects bn_acc_dscale's pattern
  auto one = [&](auto grouped, const ushort8& xv,
                 const PoolGather<K, S>& pg) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float xf = bf16_to_f32(xv[j]);
      float g = pg.grad(j);
      if (!bn_pool_relu_on(xf, sc[j], bf[j])) g = 0.f;
      adb[j] += g;
      ads[j] = bn_acc_dscale<decltype(grouped)::value>(
          ads[j], g, bn_pool_xhat(xf, mu[j], is[j]), j);
    }
  };
  long long row = rows.first(M);
  for (; row + (KS_BN_UNROLL - 1) * stride < M;
       row += KS_BN_UNROLL * stride) {
    // a real loop: unrolled, the next sub-batch's loads are hoisted over
    // this one's arithmetic and the registers run out
#pragma unroll 1
    for (int h = 0; h < KS_BN_UNROLL; h += U) {
      ushort8 xv[U];
      PoolGather<K, S> pg[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const long long r = row + (h + u) * stride;
        xv[u] = x[r * CG + cg];
        pg[u].load(dy, idx, nullptr, (int)r, H, W, OH, OW, pad, CG, cg);
      }
#pragma unroll
      for (int u = 0; u < U; u++) one(std::true_type{}, xv[u], pg[u]);
    }
  }
  for (; row < M; row += stride) {
    const ushort8 xv = x[row * CG + cg];
    PoolGather<K, S> pg;
    pg.load(dy, idx, nullptr, (int)row, H, W, OH, OW, pad, CG, cg);
    one(std::false_type{}, xv, pg);
  }

  const int C = CG * 8;
  nhwc_block_partials<KS_BN_BLOCK>(s_red, adb, part, CG);
  __syncthreads();
  nhwc_block_partials<KS_BN_BLOCK>(s_red, ads,
                                   part + (long long)gridDim.x * C, CG);
}

template <int K, int S, int U>
__global__ void __launch_bounds__(KS_BN_BLOCK)
bn_pool_bwd_apply_kernel(const ushort8* __restrict__ x,
                         const ushort8* __restrict__ dy,
                         const uint2* __restrict__ idx,
                         ushort8* __restrict__ dx,
                         const float* __restrict__ mean,
                         const float* __restrict__ invstd,
                         const float* __restrict__ weight,
                         const float* __restrict__ bias,
                         const float* __restrict__ dbias,
                         const float* __restrict__ dscale, int H, int W,
                         int OH, int OW, int pad, long long M, int CG) {
  static_assert(KS_BN_UNROLL % U == 0, "sub-batches must tile a group");
  const NhwcRows<KS_BN_BLOCK> rows(CG);
  const int cg = rows.cg;
  const long long stride = rows.stride;
  const float invM = 1.f / (float)M;
  float8 mu, is, sc, bf, db, ds;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int c = cg * 8 + j;
    mu[j] = mean[c];
    is[j] = invstd[c];
    sc[j] = bn_pool_fold_scale(weight[c], is[j]);
    bf[j] = bn_pool_fold_bias(bias[c], mu[j], sc[j]);
    db[j] = dbias[c] * invM;
    ds[j] = dscale[c] * invM;
  }
  auto one = [&](const ushort8& xv, const PoolGather<K, S>& pg) {
    ushort8 o;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float xf = bf16_to_f32(xv[j]);
      float g = pg.grad(j);
      if (!bn_pool_relu_on(xf, sc[j], bf[j])) g = 0.f;
      o[j] = f32_to_bf16(
          bn_pool_dx(sc[j], g, db[j], bn_pool_xhat(xf, mu[j], is[j]), ds[j]));
    }
    return o;
  };
  long long row = rows.first(M);
  for (; row + (KS_BN_UNROLL - 1) * stride < M;
       row += KS_BN_UNROLL * stride) {
#pragma unroll 1
    for (int h = 0; h < KS_BN_UNROLL; h += U) {
      ushort8 xv[U];
      long long k[U];
      PoolGather<K, S> pg[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const long long r = row + (h + u) * stride;
        k[u] = r * CG + cg;
        xv[u] = x[k[u]];
        pg[u].load(dy, idx, nullptr, (int)r, H, W, OH, OW, pad, CG, cg);
      }
#pragma unroll
      for (int u = 0; u < U; u++) dx[k[u]] = one(xv[u], pg[u]);
    }
  }
  for (; row < M; row += stride) {
    const long long k = row * CG + cg;
    const ushort8 xv = x[k];
    PoolGather<K, S> pg;
    pg.load(dy, idx, nullptr, (int)row, H, W, OH, OW, pad, CG, cg);
    dx[k] = one(xv, pg);
  }
}

// ================================================================== host
namespace {

struct BnPoolGeom {
  BnGeom bn;      // over the input pixels
  PoolGeom pool;  // the window arithmetic and its checks
};

BnPoolGeom bn_pool_geom(const torch::Tensor& x, int64_t k, int64_t s,
                        int64_t p) {
  pool_check_cfg("bn_relu_pool", k, s, p);
  TORCH_CHECK(x.is_cuda(), "bn_relu_pool: GPU tensor expected");
  BnPoolGeom g;
  g.bn = bn_geom_of(x);
  g.pool = pool_geom("bn_relu_pool", x.size(0), g.bn.C, x.size(2), x.size(3),
                     k, s, p);
  return g;
}

void check_params(const BnPoolGeom& g, const torch::Tensor& t,
                  const char* what) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat &&
                  t.is_contiguous() && t.numel() == g.bn.C,
              "bn_relu_pool: ", what, " must be a contiguous f32 GPU tensor "
              "of C elements");
}

// y (and the one-byte codes when idx is defined) from x and the folded
// constants
torch::Tensor launch_fwd(const torch::Tensor& x, const BnPoolGeom& g,
                         int64_t k, const torch::Tensor& scale,
                         const torch::Tensor& biasf, torch::Tensor idx,
                         hipStream_t stream) {
  auto y = at::empty({g.pool.N, g.bn.C, g.pool.OH, g.pool.OW},
                     x.options().memory_format(at::MemoryFormat::ChannelsLast));
  const bool want_idx = idx.defined();
  const unsigned int blocks = pool_blocks_for(g.pool.MO, g.bn.CG);
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(KS_POOL_BLOCK), 0, stream,
                       nhwc_cptr(x),
                       nhwc_mptr(y),
                       want_idx ? reinterpret_cast<uint2*>(idx.data_ptr())
                                : nullptr,
                       scale.data_ptr<float>(), biasf.data_ptr<float>(),
                       g.pool.H, g.pool.W, g.pool.OH, g.pool.OW, g.pool.pad,
                       (int)g.pool.MO, g.bn.CG);
  };
  if (k == 3)
    want_idx ? launch(bn_pool_fwd_kernel<3, 2, true>)
             : launch(bn_pool_fwd_kernel<3, 2, false>);
  else
    want_idx ? launch(bn_pool_fwd_kernel<2, 2, true>)
             : launch(bn_pool_fwd_kernel<2, 2, false>);
  return y;
}

}  // namespace

// Training-mode forward. Returns {y, mean, invstd} and, when want_idx,
// the codes (N, OH, OW, C) uint8 as a fourth tensor; without want_idx no
// codes tensor is allocated.
std::vector<torch::Tensor> bn_relu_pool_fwd_train(
    torch::Tensor x, torch::Tensor weight, torch::Tensor bias,
    torch::Tensor running_mean, torch::Tensor running_var, double momentum,
    double eps, int64_t k, int64_t s, int64_t p, bool want_idx,
    bool legacy_reduce) {
  BnPoolGeom g = bn_pool_geom(x, k, s, p);
  check_params(g, weight, "weight");
  check_params(g, bias, "bias");
  auto stream = at::cuda::getCurrentCUDAStream();
  auto f32 = x.options().dtype(at::kFloat);
  auto save_mean = at::empty({g.bn.C}, f32);
  auto save_invstd = at::empty({g.bn.C}, f32);
  auto scale = at::empty({g.bn.C}, f32);
  auto biasf = at::empty({g.bn.C}, f32);
  float* rmean_p =
      running_mean.defined() ? running_mean.data_ptr<float>() : nullptr;
  float* rvar_p =
      running_var.defined() ? running_var.data_ptr<float>() : nullptr;
  bn_launch_fwd_stats(x, g.bn, weight, bias, rmean_p, rvar_p, save_mean,
                      save_invstd, scale, biasf, momentum, eps, legacy_reduce,
                      stream.stream());
  torch::Tensor idx;
  if (want_idx)
    idx = at::empty({g.pool.N, g.pool.OH, g.pool.OW, g.bn.C},
                    x.options().dtype(at::kByte));
  auto y = launch_fwd(x, g, k, scale, biasf, idx, stream.stream());
  if (!want_idx) return {y, save_mean, save_invstd};
  return {y, save_mean, save_invstd, idx};
}

// Eval-mode forward (running statistics, no codes): two launches, all
// addresses in the kernel arguments, no host sync.
std::vector<torch::Tensor> bn_relu_pool_fwd_eval(
    torch::Tensor x, torch::Tensor weight, torch::Tensor bias,
    torch::Tensor rmean, torch::Tensor rvar, double eps, int64_t k,
    int64_t s, int64_t p) {
  BnPoolGeom g = bn_pool_geom(x, k, s, p);
  check_params(g, weight, "weight");
  check_params(g, bias, "bias");
  check_params(g, rmean, "running_mean");
  check_params(g, rvar, "running_var");
  auto stream = at::cuda::getCurrentCUDAStream();
  auto f32 = x.options().dtype(at::kFloat);
  auto scale = at::empty({g.bn.C}, f32);
  auto biasf = at::empty({g.bn.C}, f32);
  bn_launch_fold_eval(weight, bias, rmean, rvar, scale, biasf, g.bn.C, eps,
                      stream.stream());
  return {launch_fwd(x, g, k, scale, biasf, torch::Tensor(),
                     stream.stream())};
}

// Returns {dx, dscale, dbias}.
std::vector<torch::Tensor> bn_relu_pool_bwd(
    torch::Tensor x, torch::Tensor dy, torch::Tensor idx,
    torch::Tensor weight, torch::Tensor bias, torch::Tensor mean,
    torch::Tensor invstd, int64_t k, int64_t s, int64_t p,
    bool legacy_reduce) {
  BnPoolGeom g = bn_pool_geom(x, k, s, p);
  check_params(g, weight, "weight");
  check_params(g, bias, "bias");
  check_params(g, mean, "mean");
  check_params(g, invstd, "invstd");
  TORCH_CHECK(dy.is_cuda() && dy.dim() == 4 &&
                  dy.scalar_type() == at::kBFloat16 && dy.size(0) == g.pool.N &&
                  dy.size(1) == g.bn.C && dy.size(2) == g.pool.OH &&
                  dy.size(3) == g.pool.OW,
              "bn_relu_pool_bwd: dy must be bf16 (N, C, OH, OW)");
  TORCH_CHECK(idx.is_cuda() && idx.scalar_type() == at::kByte &&
                  idx.is_contiguous() && idx.dim() == 4 &&
                  idx.size(0) == g.pool.N && idx.size(1) == g.pool.OH &&
                  idx.size(2) == g.pool.OW && idx.size(3) == g.bn.C,
              "bn_relu_pool_bwd: idx must be uint8 (N, OH, OW, C)");
  if (!dy.is_contiguous(at::MemoryFormat::ChannelsLast))
    dy = dy.contiguous(at::MemoryFormat::ChannelsLast);
  auto stream = at::cuda::getCurrentCUDAStream();
  auto f32 = x.options().dtype(at::kFloat);
  const BnGeom& b = g.bn;
  auto part = at::empty({(long long)2 * b.stat_blocks * b.C}, f32);
  auto red = at::empty({b.C * 2}, f32);
  float* dbias_p = red.data_ptr<float>();
  float* dscale_p = dbias_p + b.C;
  auto dx = at::empty_like(x);

  auto launch_stats = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(b.stat_blocks), dim3(KS_BN_BLOCK), 0,
                       stream.stream(),
                       nhwc_cptr(x),
                       nhwc_cptr(dy),
                       reinterpret_cast<const uint2*>(idx.data_ptr()),
                       mean.data_ptr<float>(), invstd.data_ptr<float>(),
                       weight.data_ptr<float>(), bias.data_ptr<float>(),
                       part.data_ptr<float>(), g.pool.H, g.pool.W, g.pool.OH,
                       g.pool.OW, g.pool.pad,
                       b.M, b.CG);
  };
  if (k == 3)
    launch_stats(bn_pool_bwd_stats_kernel<3, 2, KS_BNP_U_321>);
  else
    launch_stats(bn_pool_bwd_stats_kernel<2, 2, KS_BNP_U_220>);
  bn_launch_bwd_reduce(part.data_ptr<float>(), b.stat_blocks, b.C, dbias_p,
                       dscale_p, legacy_reduce, stream.stream());
  auto launch_apply = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(b.blocks), dim3(KS_BN_BLOCK), 0,
                       stream.stream(),
                       nhwc_cptr(x),
                       nhwc_cptr(dy),
                       reinterpret_cast<const uint2*>(idx.data_ptr()),
                       nhwc_mptr(dx),
                       mean.data_ptr<float>(), invstd.data_ptr<float>(),
                       weight.data_ptr<float>(), bias.data_ptr<float>(),
                       dbias_p, dscale_p, g.pool.H, g.pool.W, g.pool.OH,
                       g.pool.OW, g.pool.pad, b.M,
                       b.CG);
  };
  if (k == 3)
    launch_apply(bn_pool_bwd_apply_kernel<3, 2, KS_BNP_U_321>);
  else
    launch_apply(bn_pool_bwd_apply_kernel<2, 2, KS_BNP_U_220>);
  return {dx, red.narrow(0, b.C, b.C), red.narrow(0, 0, b.C)};
}
