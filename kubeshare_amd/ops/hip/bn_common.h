// BN-specific pieces shared between bn_relu.hip, bn_pool.hip, bn_join.hip
// and bias_relu.hip: the pinned per-element expressions, the launch
// geometry and the host steps these translation units run (the kernels
// themselves live in bn_relu.hip). Types, bf16 helpers, the row walk and
// the block partials are nhwc_common.h's.
#pragma once
#include "nhwc_common.h"

#define KS_BN_BLOCK 512
#define KS_BN_UNROLL 4

// Forward apply, per element: y = bf16(relu(fma(x, scale', bias'))).
// bn_apply_relu_kernel and the pooled apply (bn_pool.hip) both go
// through these two, so a pooled output is a value the unpooled kernel
// would have written.
__device__ __forceinline__ float bn_affine(float x, float s, float b) {
  return fmaf(x, s, b);
}

__device__ __forceinline__ unsigned short bn_relu_bf16(float f) {
  return f32_to_bf16(f < 0.f ? 0.f : f);
}

// dscale accumulation, pinned. Left to -ffp-contract the backend fused
// `ads += g * xhat` for some channels and rows and not for others (it
// vectorises across rows for channels 6 and 7 of a four-row group), so
// the sums depended on the unroll. The pattern is now explicit and is
// the one every earlier build computed: within a whole group of four
// rows channels 0-5 use an FMA and channels 6-7 a rounded product, then
// an add; the leftover rows use an FMA for every channel. Any unroll
// that keeps a lane's rows in order and in the same groups of four
// therefore gives the same bits.
__device__ __forceinline__ float bn_mul_add_unfused(float acc, float a,
                                                    float b) {
#pragma clang fp contract(off)
  float prod = a * b;
  return acc + prod;
}

template <bool GROUPED>
__device__ __forceinline__ float bn_acc_dscale(float acc, float g, float xhat,
                                               int j) {
  return (GROUPED && j >= 6) ? bn_mul_add_unfused(acc, g, xhat)
                             : fmaf(g, xhat, acc);
}

// Sum of the two gradients of a forked residual join, rounded to bf16
// as a separate bf16 add kernel would have stored it.
__device__ __forceinline__ float bn_join_grad(unsigned short a,
                                              unsigned short b) {
  return bf16_to_f32(f32_to_bf16(bf16_to_f32(a) + bf16_to_f32(b)));
}

// xhat = (x - mean) * invstd: a subtraction, then a product
__device__ __forceinline__ float bn_pool_xhat(float xf, float mu, float is) {
#pragma clang fp contract(off)
  return (xf - mu) * is;
}

// dx = w' * (g - dbias/M - xhat * dscale/M), pinned: one subtraction,
// one FMA, one product
__device__ __forceinline__ float bn_pool_dx(float w, float g, float db,
                                            float xhat, float ds) {
#pragma clang fp contract(off)
  const float t = g - db;
  return w * fmaf(-xhat, ds, t);
}

// ReLU mask of one lane's 8 stored bf16 values: bit j is set iff value j
// is > 0, the predicate the backward applies to y (a NaN gives 0).
__device__ __forceinline__ unsigned char bn_mask_byte(const ushort8& o) {
  unsigned int m = 0;
#pragma unroll
  for (int j = 0; j < 8; j++)
    m |= (bf16_to_f32(o[j]) > 0.f ? 1u : 0u) << j;
  return (unsigned char)m;
}

// ------------------------------------------------------------------ host
struct BnGeom {
  long long M;  // rows (N*H*W)
  int C, CG, blocks, stat_blocks;
};

// Checks x (4-D bf16 channels-last, C % 8 == 0, C <= 8*KS_BN_BLOCK) and
// sizes the grid-stride launches: `blocks` for the apply kernels,
// `stat_blocks` for the kernels that leave block partials.
BnGeom bn_geom_of(const torch::Tensor& x);

// Checks the byte mask of bn_mask_byte against x: contiguous uint8 of
// shape (N, H, W, C/8) on the GPU.
void bn_check_mask(const torch::Tensor& mask, const torch::Tensor& x,
                   const BnGeom& g);

// Forward statistics of a training step: bn_stats_kernel, then
// bn_reduce_tile_kernel<.., true> (legacy_reduce: the earlier reduce and
// finalize kernels). Leaves mean/invstd in save_*, the folded scale' and
// bias' in scale/biasf, and updates the running statistics when the
// pointers are non-null.
void bn_launch_fwd_stats(const torch::Tensor& x, const BnGeom& g,
                         const torch::Tensor& weight,
                         const torch::Tensor& bias, float* running_mean,
                         float* running_var, torch::Tensor& save_mean,
                         torch::Tensor& save_invstd, torch::Tensor& scale,
                         torch::Tensor& biasf, double momentum, double eps,
                         bool legacy_reduce, hipStream_t stream);

// Block partials part[2][nblocks][C] -> out0[C], out1[C]:
// bn_reduce_tile_kernel<.., false>, or the legacy kernel.
void bn_launch_bwd_reduce(const float* part, int nblocks, int C, float* out0,
                          float* out1, bool legacy_reduce,
                          hipStream_t stream);

// Block partials part[nblocks][C] -> out[C]: the one-output form of
// bn_reduce_tile_kernel<.., false> (same summation contract, half the
// loads of the two-slot form).
void bn_launch_reduce_one(const float* part, int nblocks, int C, float* out,
                          hipStream_t stream);

// Eval mode: scale' and bias' from the running statistics
// (bn_fold_eval_kernel).
void bn_launch_fold_eval(const torch::Tensor& weight,
                         const torch::Tensor& bias,
                         const torch::Tensor& rmean,
                         const torch::Tensor& rvar, torch::Tensor& scale,
                         torch::Tensor& biasf, int C, double eps,
                         hipStream_t stream);
