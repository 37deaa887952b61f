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
// Conventions are bn_relu.hip's and pool.hip's: one lane owns 8
// consecutive channels (one 16-byte access), 64-bit element offsets,
// 32-bit pixel indices (the host checks N*H*W < 2**31), tail threads
// idle when C/8 does not divide the block. Every floating-point
// expression whose contraction could differ between instantiations is
// written with explicit fmaf or under contract(off).
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <vector>

#include "bn_common.h"

#define KS_BNP_FWD_BLOCK 256  // pool.hip's KS_POOL_BLOCK
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
__global__ void __launch_bounds__(KS_BNP_FWD_BLOCK)
bn_pool_fwd_kernel(const ushort8* __restrict__ x, ushort8* __restrict__ y,
                   uint2* __restrict__ idx, const float* __restrict__ scale,
                   const float* __restrict__ biasf, int H, int W, int OH,
                   int OW, int pad, int M, int CG) {
  const int tid = threadIdx.x;
  const int cg = tid % CG;
  const int roff = tid / CG;
  const int rows_per_blk = KS_BNP_FWD_BLOCK / CG;
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
  float8 s, b;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    s[j] = scale[cg * 8 + j];
    b[j] = biasf[cg * 8 + j];
  }

  // pool.hip's rule: start from -inf at the first in-bounds position
  // (pad < K: there is one), take a value if val > best || isnan(val),
  // row-major
  const unsigned int q0 =
      (unsigned int)((h0 < 0 ? -h0 : 0) * K + (w0 < 0 ? -w0 : 0));
  float best[8];
  unsigned int code[8];
  ushort8 o;
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
        // the value bn_apply_relu_kernel<false, true> would have stored
        const unsigned short yb =
            bn_relu_bf16(bn_affine(bf16_to_f32(v[q][j]), s[j], b[j]));
        const float f = bf16_to_f32(yb);
        if (f > best[j] || f != f) {
          best[j] = f;
          o[j] = yb;
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
// What one lane needs to form the pool gradient of 8 channels of one
// input pixel: max_pool_nhwc_bwd_kernel's loads and bookkeeping, kept
// apart from the arithmetic so that a sub-batch can issue all its loads
// first.
template <int K, int S>
struct PoolGather {
  static constexpr int NW = (K + S - 1) / S;
  ushort8 g[NW * NW];
  uint2 c[NW * NW];
  unsigned int want[NW * NW];
  bool ok[NW * NW];

  // row = input pixel (n, h, w) < N*H*W
  __device__ __forceinline__ void load(const ushort8* __restrict__ dy,
                                       const uint2* __restrict__ idx,
                                       int row, int H, int W, int OH, int OW,
                                       int pad, int CG, int cg) {
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
        want[q] =
            (unsigned int)((h + pad - oh * S) * K + (w + pad - ow * S));
        const long long k =
            (((long long)n * OH + ohc) * OW + owc) * CG + cg;
        g[q] = dy[k];
        c[q] = idx[k];
      }
    }
  }

  // channel j's pool gradient as the unfused backward would have
  // stored it: f32 sum in ascending (oh, ow) order, one RNE rounding
  __device__ __forceinline__ float grad(int j) const {
    float acc = 0.f;
#pragma unroll
    for (int q = 0; q < NW * NW; q++) {
      if (ok[q]) {
        const unsigned int word = j < 4 ? c[q].x : c[q].y;
        const unsigned int code = (word >> (8 * (j & 3))) & 0xffu;
        if (code == want[q]) acc += bf16_to_f32(g[q][j]);
      }
    }
    return bf16_to_f32(f32_to_bf16(acc));
  }
};

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
  const int tid = threadIdx.x;
  const int cg = tid % CG;
  const int roff = tid / CG;
  const int rows_per_blk = KS_BN_BLOCK / CG;
  const bool active = roff < rows_per_blk;  // see bn_stats_kernel
  const long long stride = (long long)gridDim.x * rows_per_blk;
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
  long long row = active ? (long long)blockIdx.x * rows_per_blk + roff : M;
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
        pg[u].load(dy, idx, (int)r, H, W, OH, OW, pad, CG, cg);
      }
#pragma unroll
      for (int u = 0; u < U; u++)
#pragma unroll
        for (int j = 0; j < 8; j++) {
          const float xf = bf16_to_f32(xv[u][j]);
          float g = pg[u].grad(j);
          if (!bn_pool_relu_on(xf, sc[j], bf[j])) g = 0.f;
          adb[j] += g;
          ads[j] = bn_acc_dscale<true>(ads[j], g,
                                       bn_pool_xhat(xf, mu[j], is[j]), j);
        }
    }
  }
  for (; row < M; row += stride) {
    const ushort8 xv = x[row * CG + cg];
    PoolGather<K, S> pg;
    pg.load(dy, idx, (int)row, H, W, OH, OW, pad, CG, cg);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float xf = bf16_to_f32(xv[j]);
      float g = pg.grad(j);
      if (!bn_pool_relu_on(xf, sc[j], bf[j])) g = 0.f;
      adb[j] += g;
      ads[j] = bn_acc_dscale<false>(ads[j], g,
                                    bn_pool_xhat(xf, mu[j], is[j]), j);
    }
  }

  // LDS tree over the lanes sharing a channel group (bn_stats_kernel's)
  const int C = CG * 8;
  float* db_part = part + (long long)blockIdx.x * C;
  float* ds_part = part + (long long)(gridDim.x + blockIdx.x) * C;
#pragma unroll
  for (int j = 0; j < 8; j++) s_red[tid * 8 + j] = adb[j];
  __syncthreads();
  if (tid < CG) {
    float8 t = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int r = 0; r < rows_per_blk; r++)
#pragma unroll
      for (int j = 0; j < 8; j++) t[j] += s_red[(r * CG + tid) * 8 + j];
#pragma unroll
    for (int j = 0; j < 8; j++) db_part[tid * 8 + j] = t[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 8; j++) s_red[tid * 8 + j] = ads[j];
  __syncthreads();
  if (tid < CG) {
    float8 t = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int r = 0; r < rows_per_blk; r++)
#pragma unroll
      for (int j = 0; j < 8; j++) t[j] += s_red[(r * CG + tid) * 8 + j];
#pragma unroll
    for (int j = 0; j < 8; j++) ds_part[tid * 8 + j] = t[j];
  }
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
  const int tid = threadIdx.x;
  const int cg = tid % CG;
  const int roff = tid / CG;
  const int rows_per_blk = KS_BN_BLOCK / CG;
  const bool active = roff < rows_per_blk;
  const long long stride = (long long)gridDim.x * rows_per_blk;
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
  long long row = active ? (long long)blockIdx.x * rows_per_blk + roff : M;
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
        pg[u].load(dy, idx, (int)r, H, W, OH, OW, pad, CG, cg);
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        ushort8 o;
#pragma unroll
        for (int j = 0; j < 8; j++) {
          const float xf = bf16_to_f32(xv[u][j]);
          float g = pg[u].grad(j);
          if (!bn_pool_relu_on(xf, sc[j], bf[j])) g = 0.f;
          o[j] = f32_to_bf16(bn_pool_dx(
              sc[j], g, db[j], bn_pool_xhat(xf, mu[j], is[j]), ds[j]));
        }
        dx[k[u]] = o;
      }
    }
  }
  for (; row < M; row += stride) {
    const long long k = row * CG + cg;
    const ushort8 xv = x[k];
    PoolGather<K, S> pg;
    pg.load(dy, idx, (int)row, H, W, OH, OW, pad, CG, cg);
    ushort8 o;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float xf = bf16_to_f32(xv[j]);
      float g = pg.grad(j);
      if (!bn_pool_relu_on(xf, sc[j], bf[j])) g = 0.f;
      o[j] = f32_to_bf16(
          bn_pool_dx(sc[j], g, db[j], bn_pool_xhat(xf, mu[j], is[j]), ds[j]));
    }
    dx[k] = o;
  }
}

// ================================================================== host
namespace {

struct BnPoolGeom {
  BnGeom bn;  // over the input pixels
  int N, H, W, OH, OW, pad;
  long long MO;  // output pixels
};

BnPoolGeom bn_pool_geom(const torch::Tensor& x, int64_t k, int64_t s,
                        int64_t p) {
  TORCH_CHECK((k == 3 && s == 2 && p == 1) || (k == 2 && s == 2 && p == 0),
              "bn_relu_pool: (k, s, p) must be (3, 2, 1) or (2, 2, 0)");
  TORCH_CHECK(x.is_cuda(), "bn_relu_pool: GPU tensor expected");
  BnPoolGeom g;
  g.bn = bn_geom_of(x);
  const int64_t N = x.size(0), H = x.size(2), W = x.size(3);
  // one 256-thread forward block spans a pixel's channel groups
  TORCH_CHECK(g.bn.C >= 8 && g.bn.C <= KS_BNP_FWD_BLOCK * 8,
              "bn_relu_pool: C must be a multiple of 8 in [8, 2048]");
  TORCH_CHECK(N >= 1 && H + 2 * p >= k && W + 2 * p >= k,
              "bn_relu_pool: empty output");
  TORCH_CHECK(N * H * W < (1LL << 31),
              "bn_relu_pool: N*H*W must fit 32 bits");
  g.N = (int)N;
  g.H = (int)H;
  g.W = (int)W;
  g.OH = (int)((H + 2 * p - k) / s + 1);
  g.OW = (int)((W + 2 * p - k) / s + 1);
  g.pad = (int)p;
  g.MO = (long long)g.N * g.OH * g.OW;
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
  auto y = at::empty({g.N, g.bn.C, g.OH, g.OW},
                     x.options().memory_format(at::MemoryFormat::ChannelsLast));
  const bool want_idx = idx.defined();
  const int rows_per_blk = KS_BNP_FWD_BLOCK / g.bn.CG;
  const unsigned int blocks =
      (unsigned int)((g.MO + rows_per_blk - 1) / rows_per_blk);
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(KS_BNP_FWD_BLOCK), 0, stream,
                       reinterpret_cast<const ushort8*>(x.data_ptr()),
                       reinterpret_cast<ushort8*>(y.data_ptr()),
                       want_idx ? reinterpret_cast<uint2*>(idx.data_ptr())
                                : nullptr,
                       scale.data_ptr<float>(), biasf.data_ptr<float>(), g.H,
                       g.W, g.OH, g.OW, g.pad, (int)g.MO, g.bn.CG);
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
    idx = at::empty({g.N, g.OH, g.OW, g.bn.C}, x.options().dtype(at::kByte));
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
                  dy.scalar_type() == at::kBFloat16 && dy.size(0) == g.N &&
                  dy.size(1) == g.bn.C && dy.size(2) == g.OH &&
                  dy.size(3) == g.OW,
              "bn_relu_pool_bwd: dy must be bf16 (N, C, OH, OW)");
  TORCH_CHECK(idx.is_cuda() && idx.scalar_type() == at::kByte &&
                  idx.is_contiguous() && idx.dim() == 4 &&
                  idx.size(0) == g.N && idx.size(1) == g.OH &&
                  idx.size(2) == g.OW && idx.size(3) == g.bn.C,
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
                       reinterpret_cast<const ushort8*>(x.data_ptr()),
                       reinterpret_cast<const ushort8*>(dy.data_ptr()),
                       reinterpret_cast<const uint2*>(idx.data_ptr()),
                       mean.data_ptr<float>(), invstd.data_ptr<float>(),
                       weight.data_ptr<float>(), bias.data_ptr<float>(),
                       part.data_ptr<float>(), g.H, g.W, g.OH, g.OW, g.pad,
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
                       reinterpret_cast<const ushort8*>(x.data_ptr()),
                       reinterpret_cast<const ushort8*>(dy.data_ptr()),
                       reinterpret_cast<const uint2*>(idx.data_ptr()),
                       reinterpret_cast<ushort8*>(dx.data_ptr()),
                       mean.data_ptr<float>(), invstd.data_ptr<float>(),
                       weight.data_ptr<float>(), bias.data_ptr<float>(),
                       dbias_p, dscale_p, g.H, g.W, g.OH, g.OW, g.pad, b.M,
                       b.CG);
  };
  if (k == 3)
    launch_apply(bn_pool_bwd_apply_kernel<3, 2, KS_BNP_U_321>);
  else
    launch_apply(bn_pool_bwd_apply_kernel<2, 2, KS_BNP_U_220>);
  return {dx, red.narrow(0, b.C, b.C), red.narrow(0, 0, b.C)};
}
