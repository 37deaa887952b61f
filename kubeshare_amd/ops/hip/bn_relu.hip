// Fused NHWC bf16 BatchNorm + ReLU (+ residual add) for gfx950.
//
// Motivation (profiles/resnet50_bs256_kernel_breakdown_untuned.txt):
// MIOpen's spatial BN kernels + separate ReLU/add elementwise passes
// are ~48% of the non-conv GPU time of a ResNet50 training step. The
// stock path makes 5 full passes over the activation in forward and 8
// in backward; these kernels make 3 forward and 5 (non-residual) / 7
// (residual) backward, and fold the residual add and its gradient for
// free. Where the output of a residual BN feeds two consumers, the
// backward also takes their two gradients separately and sums them in
// registers (one extra read, 7+1 passes) instead of autograd's separate
// bf16 add kernel (three passes) — see bn_bwd_stats_kernel.
//
// Design (cdna_hip_programming.md G13 vectorize, G7 ILP, G11 grid):
//  - channels-last bf16, C % 8 == 0: one lane owns 8 CONSECUTIVE
//    channels (one 16-byte load) — per-channel reductions never cross
//    lanes, and a wave's 64 lanes cover a 1 KiB contiguous span.
//  - UNROLL independent row-chunks per loop iteration so each lane
//    keeps >=4 16-B loads in flight (1 load/lane measured ~2.3 TB/s,
//    HBM-latency-bound at 32 waves/CU).
//  - block partials + a tree-reduce in a second kernel instead of
//    per-channel global atomics (2*C atomics x 2048 blocks measured as
//    ~0.4 ms of fixed cost per BN call).
//  - all stats/parameter math in f32; tensors read/written as bf16x8.
//  - the row walk with its idle-tail rule (NhwcRows) and the LDS tree of
//    the block partials (nhwc_block_partials) are nhwc_common.h's; each
//    kernel writes its per-row arithmetic once, as `one(...)`.
//
// Launch sequence (three launches each):
//   forward   bn_stats -> bn_reduce_tile<FINALIZE> -> bn_apply_relu
//   backward  bn_bwd_stats[_noy] -> bn_reduce_tile -> bn_bwd_apply_*
// The stats kernels leave part[b*C + c] (second half at + nblocks*C);
// bn_reduce_tile_kernel sums it over b with its lanes along c (coalesced)
// and, in forward, goes straight on to the per-channel finalize math.
// Reduce contract, per channel and half: 64 accumulators a[L] take the
// blocks b = L, L+64, ... in ascending order, then a[i] += a[i+off] for
// off = 32 .. 1; see bn_reduce_tile_kernel. legacy_reduce=true (Python:
// KUBESHARE_BN_REDUCE=legacy) runs the earlier bn_reduce_partials_kernel
// (+ bn_finalize_kernel in forward) instead: same sums bit for bit, one
// wave per channel reading 4 bytes of each of 64 rows per instruction.
// It is the oracle of tests/test_bn_reduce_gpu.py and the A/B baseline.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <type_traits>
#include <vector>

// KS_BN_BLOCK / KS_BN_UNROLL, the pinned per-element expressions and the
// host steps shared with the other BN files; through it nhwc_common.h:
// types, bf16 helpers, the row walk (NhwcRows) and the block partials
#include "bn_common.h"

#define KS_BN_UNROLL_STATS 8
// two-gradient bwd stats: rows loaded per sub-batch of a KS_BN_UNROLL
// group (see bn_bwd_stats_kernel)
#define KS_BN_UNROLL_DY2 2

// ------------------------------------------------------------- fwd stats
// Block partials: sum_part[b*C + c], sq_part[(B + b)*C + c].
__global__ void bn_stats_kernel(const ushort8* __restrict__ x,
                                float* __restrict__ part,
                                long long M, int CG) {
  __shared__ float s_red[KS_BN_BLOCK * 8];
  const NhwcRows<KS_BN_BLOCK> rows(CG);
  const int cg = rows.cg;
  const long long stride = rows.stride;

  float8 acc = {0, 0, 0, 0, 0, 0, 0, 0};
  float8 acc2 = {0, 0, 0, 0, 0, 0, 0, 0};
  auto one = [&](const ushort8& v) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
      float f = bf16_to_f32(v[j]);
      acc[j] += f;
      acc2[j] += f * f;
    }
  };
  long long row = rows.first(M);
  // unrolled main loop: KS_BN_UNROLL_STATS independent loads in flight
  for (; row + (KS_BN_UNROLL_STATS - 1) * stride < M;
       row += KS_BN_UNROLL_STATS * stride) {
    ushort8 v[KS_BN_UNROLL_STATS];
#pragma unroll
    for (int u = 0; u < KS_BN_UNROLL_STATS; u++)
      v[u] = x[(row + u * stride) * CG + cg];
#pragma unroll
    for (int u = 0; u < KS_BN_UNROLL_STATS; u++) one(v[u]);
  }
  for (; row < M; row += stride) {
    ushort8 v = x[row * CG + cg];
    one(v);
  }

  const int C = CG * 8;
  nhwc_block_partials<KS_BN_BLOCK>(s_red, acc, part, CG);
  __syncthreads();
  nhwc_block_partials<KS_BN_BLOCK>(s_red, acc2,
                                   part + (long long)gridDim.x * C, CG);
}

// ---------------------------------------- partial reduction (legacy)
// part[b*C + c] (+ the sq/dscale half at offset nblocks*C) -> out[c].
// Kept for legacy_reduce=true; bn_reduce_tile_kernel replaces it.
// One 64-lane wave per 4 channels: lanes stride over blocks (all loads
// independent -> one latency, not nblocks of them), then shfl-reduce.
__global__ void bn_reduce_partials_kernel(const float* __restrict__ part,
                                          int nblocks, int C,
                                          float* __restrict__ out0,
                                          float* __restrict__ out1) {
  const int lane = threadIdx.x;        // 0..63 over blocks
  const int c = blockIdx.x * blockDim.y + threadIdx.y;
  if (c >= C) return;
  float a0 = 0.f, a1 = 0.f;
  for (int b = lane; b < nblocks; b += 64) {
    a0 += part[(long long)b * C + c];
    a1 += part[(long long)(nblocks + b) * C + c];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a0 += __shfl_down(a0, off, 64);
    a1 += __shfl_down(a1, off, 64);
  }
  if (lane == 0) {
    out0[c] = a0;
    out1[c] = a1;
  }
}

// ------------------------------------------------------- fwd finalize
// One channel's mean/invstd, running-stat update (PyTorch semantics) and
// folded scale' = w*invstd, bias' = b - mean*s, from its two sums.
// Pinned: left to -ffp-contract, which of these expressions become FMAs
// depends on the kernel they are inlined into. The sequence written out
// here is the one the stand-alone bn_finalize_kernel always compiled to
// (read from its ISA): var and bias' use an FMA, the running-stat
// updates two rounded products and an add.
struct BnFinalizeArgs {
  const float* __restrict__ weight;
  const float* __restrict__ bias;
  float* __restrict__ running_mean;  // may be null (with running_var)
  float* __restrict__ running_var;
  float* __restrict__ save_mean;
  float* __restrict__ save_invstd;
  float* __restrict__ scale_out;
  float* __restrict__ bias_out;
  long long M;
  float momentum, eps;
};

__device__ __forceinline__ void bn_finalize_channel(const BnFinalizeArgs& f,
                                                    int c, float sum,
                                                    float sumsq) {
#pragma clang fp contract(off)
  const long long M = f.M;
  float mean = sum / (float)M;
  float var = fmaf(-mean, mean, sumsq / (float)M);
  var = var < 0.f ? 0.f : var;
  float invstd = rsqrtf(var + f.eps);
  f.save_mean[c] = mean;
  f.save_invstd[c] = invstd;
  if (f.running_mean) {
    float unbiased = M > 1 ? var * (float)M / (float)(M - 1) : var;
    const float keep = 1.f - f.momentum;
    float rm = keep * f.running_mean[c];
    float rv = keep * f.running_var[c];
    float nm = f.momentum * mean;
    float nv = f.momentum * unbiased;
    f.running_mean[c] = rm + nm;
    f.running_var[c] = rv + nv;
  }
  float s = f.weight[c] * invstd;
  f.scale_out[c] = s;
  f.bias_out[c] = fmaf(-mean, s, f.bias[c]);
}

// ------------------------------------- coalesced reduce (+ fwd finalize)
// Same sums as bn_reduce_partials_kernel, bit for bit, with the lanes
// running along CHANNELS: a block owns TILE consecutive channels and 64
// accumulators per channel and half, so a wave instruction reads
// 64/TILE rows of TILE*4 contiguous bytes instead of 64 rows of 4.
//
// Contract (per channel, separately for the two halves of `part`):
//   a[L] = 0.f; a[L] += part[b][c] for b = L, L+64, L+128, ... ascending
//   for off in 32,16,8,4,2,1: a[i] += a[i+off] for i < off
//   result = a[0]
// which is the legacy kernel's __shfl_down tree as lane 0 sees it.
//
// Mapping: thread = (wave w, k, cc) with lane = k*TILE + cc and
// L = w + NW*k (NW = TILE waves per block). The tree steps off >= NW
// pair accumulators of one wave (lane distance off/NW*TILE: shuffles);
// the NW survivors per channel go through LDS to a second set of
// shuffles in which lane = L*QC + q carries channel wave*QC + q.
// FINALIZE: the lanes that end up with a channel's two sums go straight
// on to bn_finalize_channel (no `sums` buffer, no finalize launch).
// TWO=false: `part` has one half only (part[nblocks][C] -> out0[C]); the
// second half's loads, shuffles and store are compiled out, the first
// half's sum is the same (bias_relu.hip's bias gradient).
// Swept in the ResNet50 bs256 step (average us per call, forward /
// backward): TILE 16 x 8 loads 7.5 / 6.8, TILE 16 x 16 loads 7.8 / 6.9,
// TILE 8 x 8 loads 7.9 / 7.0 — flat; what is left is mostly the cost
// of a dependent launch (bn_finalize_kernel alone took 4.8).
#define KS_BN_RTILE 16
#define KS_BN_RLOADS 8  // independent loads in flight per half and thread

template <int TILE, bool FINALIZE, bool TWO = true>
__global__ void __launch_bounds__(64 * TILE)
bn_reduce_tile_kernel(const float* __restrict__ part, int nblocks, int C,
                      float* __restrict__ out0, float* __restrict__ out1,
                      const BnFinalizeArgs fin) {
  constexpr int NW = TILE;       // waves per block
  constexpr int QC = 64 / NW;    // channels per wave in the second stage
  static_assert(TILE == 8 || TILE == 16, "64 % TILE, 64 * TILE <= 1024");
  static_assert(TWO || !FINALIZE, "the finalize math needs both sums");
  __shared__ float s_a[2][NW][TILE];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int cc = lane % TILE;
  const int L = w + NW * (lane / TILE);
  const int c = blockIdx.x * TILE + cc;
  const bool valid = c < C;  // C % 8 == 0: the last tile may be partial
  const float* p0 = part + c;
  const float* p1 = part + (long long)nblocks * C + c;
  float a0 = 0.f, a1 = 0.f;
  for (int b0 = L; b0 < nblocks; b0 += 64 * KS_BN_RLOADS) {
    float v0[KS_BN_RLOADS], v1[KS_BN_RLOADS];
#pragma unroll
    for (int u = 0; u < KS_BN_RLOADS; u++) {
      const int b = b0 + 64 * u;
      const bool ok = valid && b < nblocks;
      v0[u] = ok ? p0[(long long)b * C] : 0.f;
      if (TWO) v1[u] = ok ? p1[(long long)b * C] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < KS_BN_RLOADS; u++)
      if (b0 + 64 * u < nblocks) {
        a0 += v0[u];
        if (TWO) a1 += v1[u];
      }
  }
  // tree steps 32 .. NW inside the wave
#pragma unroll
  for (int off = 32; off >= NW; off >>= 1) {
    a0 += __shfl_down(a0, off / NW * TILE, 64);
    if (TWO) a1 += __shfl_down(a1, off / NW * TILE, 64);
  }
  if (lane < TILE) {  // L == w: a[0 .. NW-1] of channel cc
    s_a[0][w][cc] = a0;
    if (TWO) s_a[1][w][cc] = a1;
  }
  __syncthreads();
  if (tid >= 64 * (TILE / QC)) return;  // whole waves leave
  const int l2 = lane / QC;             // 0 .. NW-1
  const int cc2 = w * QC + lane % QC;
  a0 = s_a[0][l2][cc2];
  if (TWO) a1 = s_a[1][l2][cc2];
#pragma unroll
  for (int off = NW / 2; off > 0; off >>= 1) {
    a0 += __shfl_down(a0, off * QC, 64);
    if (TWO) a1 += __shfl_down(a1, off * QC, 64);
  }
  const int c2 = blockIdx.x * TILE + cc2;
  if (l2 != 0 || c2 >= C) return;
  if (FINALIZE) {
    bn_finalize_channel(fin, c2, a0, a1);
  } else {
    out0[c2] = a0;
    if (TWO) out1[c2] = a1;
  }
}

// Legacy finalize launch (KUBESHARE_BN_REDUCE=legacy), after
// bn_reduce_partials_kernel.
__global__ void bn_finalize_kernel(const float* __restrict__ sum,
                                   const float* __restrict__ sumsq,
                                   const float* __restrict__ weight,
                                   const float* __restrict__ bias,
                                   float* __restrict__ running_mean,
                                   float* __restrict__ running_var,
                                   float* __restrict__ save_mean,
                                   float* __restrict__ save_invstd,
                                   float* __restrict__ scale_out,
                                   float* __restrict__ bias_out,
                                   long long M, int C, float momentum,
                                   float eps) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const BnFinalizeArgs f = {weight, bias, running_mean, running_var,
                            save_mean, save_invstd, scale_out, bias_out,
                            M, momentum, eps};
  bn_finalize_channel(f, c, sum[c], sumsq[c]);
}

// --------------------------------------------------------- fwd apply
// y = [relu](x*scale' + bias' [+ res]); scale/bias in registers.
// RELU=false serves the reference ResNet's downsample-path BNs (no
// activation), which otherwise fall back to MIOpen's fp32 spatial BN.
// MASK: also leaves the ReLU mask of each lane's 8 stored values as one
// byte per lane and row (bn_mask_byte), for the backward to read instead
// of y.
template <bool WITH_RES, bool RELU = true, bool MASK = false>
__global__ void bn_apply_relu_kernel(const ushort8* __restrict__ x,
                                     const ushort8* __restrict__ res,
                                     ushort8* __restrict__ y,
                                     unsigned char* __restrict__ mask,
                                     const float* __restrict__ scale,
                                     const float* __restrict__ biasf,
                                     long long M, int CG) {
  const NhwcRows<KS_BN_BLOCK> rows(CG);
  const int cg = rows.cg;
  const long long stride = rows.stride;
  float8 s, b;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    s[j] = scale[cg * 8 + j];
    b[j] = biasf[cg * 8 + j];
  }
  // one row: r is read only WITH_RES
  auto one = [&](long long k, const ushort8& v, const ushort8& r) {
    ushort8 o;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      float f = bn_affine(bf16_to_f32(v[j]), s[j], b[j]);
      if (WITH_RES) f += bf16_to_f32(r[j]);
      o[j] = RELU ? bn_relu_bf16(f) : f32_to_bf16(f);
    }
    y[k] = o;
    if (MASK) mask[k] = bn_mask_byte(o);
  };
  long long row = rows.first(M);
  for (; row + (KS_BN_UNROLL - 1) * stride < M;
       row += KS_BN_UNROLL * stride) {
    ushort8 v[KS_BN_UNROLL], r[KS_BN_UNROLL];
    long long k[KS_BN_UNROLL];
#pragma unroll
    for (int u = 0; u < KS_BN_UNROLL; u++) {
      k[u] = (row + u * stride) * CG + cg;
      v[u] = x[k[u]];
      if (WITH_RES) r[u] = res[k[u]];
    }
#pragma unroll
    for (int u = 0; u < KS_BN_UNROLL; u++) one(k[u], v[u], r[u]);
  }
  for (; row < M; row += stride) {
    const long long k = row * CG + cg;
    ushort8 v = x[k];
    ushort8 r;
    if (WITH_RES) r = res[k];
    one(k, v, r);
  }
}

// --------------------------------------------------------- bwd stats
// dym = dy * (y > 0); dbias[c] = sum(dym); dscale[c] = sum(dym*xhat);
// optionally writes dym (= the residual branch's gradient).
// WITH_DY2: y fed two consumers (the next block's conv1 and its identity
// branch) and their gradients arrive separately; the join sum
// bf16(f32(dy) + f32(dy2)) is formed in registers — bit-for-bit what a
// separate bf16 add kernel would have written and this kernel re-read.
// MASK: the predicate y > 0 comes from the byte the forward apply left
// per lane and row (bn_mask_byte) instead of from y itself: 1/16 of a
// pass instead of a whole one, the same bits out.
// (bn_join_grad and the pinned dscale accumulation, bn_acc_dscale, are
// in bn_common.h)
template <bool WRITE_DYM, bool WITH_DY2 = false, bool MASK = false>
__global__ void bn_bwd_stats_kernel(const ushort8* __restrict__ x,
                                    const ushort8* __restrict__ y,
                                    const unsigned char* __restrict__ mask,
                                    const ushort8* __restrict__ dy,
                                    const ushort8* __restrict__ dy2,
                                    ushort8* __restrict__ dym_out,
                                    const float* __restrict__ mean,
                                    const float* __restrict__ invstd,
                                    float* __restrict__ part,
                                    long long M, int CG) {
  __shared__ float s_red[KS_BN_BLOCK * 8];
  const NhwcRows<KS_BN_BLOCK> rows(CG);
  const int cg = rows.cg;
  const long long stride = rows.stride;
  float8 mu, is;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    mu[j] = mean[cg * 8 + j];
    is[j] = invstd[cg * 8 + j];
  }
  float8 adb = {0, 0, 0, 0, 0, 0, 0, 0};
  float8 ads = {0, 0, 0, 0, 0, 0, 0, 0};
  // one row; `grouped` (std::true_type inside a whole group of four
  // rows) selects bn_acc_dscale's pattern. yv is read only without
  // MASK, mv only with it, g2 only WITH_DY2.
  auto one = [&](auto grouped, long long k, const ushort8& xv,
                 const ushort8& yv, const unsigned char& mv,
                 const ushort8& gv, const ushort8& g2) {
    ushort8 dm;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      float gin = WITH_DY2 ? bn_join_grad(gv[j], g2[j]) : bf16_to_f32(gv[j]);
      const bool on = MASK ? ((mv >> j) & 1) != 0 : bf16_to_f32(yv[j]) > 0.f;
      float g = on ? gin : 0.f;
      float xhat = (bf16_to_f32(xv[j]) - mu[j]) * is[j];
      adb[j] += g;
      ads[j] = bn_acc_dscale<decltype(grouped)::value>(ads[j], g, xhat, j);
      if (WRITE_DYM) dm[j] = f32_to_bf16(g);
    }
    if (WRITE_DYM) dym_out[k] = dm;
  };
  // Rows advance in groups of KS_BN_UNROLL; a group is loaded U rows at
  // a time. The two-gradient variant reads four tensors per row instead
  // of three, and at U = KS_BN_UNROLL it spills (112 B/lane of scratch
  // under the 128-VGPR budget); two rows at a time it does not.
  // (MASK, one gradient: 76 B/lane of scratch at U = KS_BN_UNROLL, none
  // at two rows; the one-gradient y-reading variant is left as it was)
  constexpr int U = (WITH_DY2 || MASK) ? KS_BN_UNROLL_DY2 : KS_BN_UNROLL;
  static_assert(KS_BN_UNROLL % U == 0, "sub-batches must tile a group");
  long long row = rows.first(M);
  for (; row + (KS_BN_UNROLL - 1) * stride < M;
       row += KS_BN_UNROLL * stride) {
    // a real loop: unrolled, the scheduler hoists the next sub-batch's
    // loads over this one's arithmetic and the spill is back
#pragma unroll 1
    for (int h = 0; h < KS_BN_UNROLL; h += U) {
      ushort8 xv[U], yv[U], gv[U];
      ushort8 g2[U];
      unsigned char mv[U];
      long long k[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        k[u] = (row + (h + u) * stride) * CG + cg;
        xv[u] = x[k[u]];
        if (MASK) mv[u] = mask[k[u]]; else yv[u] = y[k[u]];
        gv[u] = dy[k[u]];
        if (WITH_DY2) g2[u] = dy2[k[u]];
      }
#pragma unroll
      for (int u = 0; u < U; u++)
        one(std::true_type{}, k[u], xv[u], yv[u], mv[u], gv[u], g2[u]);
    }
  }
  for (; row < M; row += stride) {
    const long long k = row * CG + cg;
    ushort8 xv = x[k], gv = dy[k];
    ushort8 yv;
    unsigned char mv;
    if (MASK) mv = mask[k]; else yv = y[k];
    ushort8 g2;
    if (WITH_DY2) g2 = dy2[k];
    one(std::false_type{}, k, xv, yv, mv, gv, g2);
  }

  const int C = CG * 8;
  nhwc_block_partials<KS_BN_BLOCK>(s_red, adb, part, CG);
  __syncthreads();
  nhwc_block_partials<KS_BN_BLOCK>(s_red, ads,
                                   part + (long long)gridDim.x * C, CG);
}

// ----------------------------------------- bwd stats, no-y variant
// Non-residual BNs: the ReLU mask is recomputed from x and the folded
// per-channel constants (y>0 <=> bf16(relu(s*x+b)) != 0, replicating
// the forward's rounding exactly), so the backward never re-reads y:
// 7 tensor passes -> 5 for the non-residual blocks of ResNet50.
// RELU=false (downsample BNs): no mask, g = dy.
template <bool RELU = true>
__global__ void bn_bwd_stats_noy_kernel(const ushort8* __restrict__ x,
                                        const ushort8* __restrict__ dy,
                                        const float* __restrict__ mean,
                                        const float* __restrict__ invstd,
                                        const float* __restrict__ weight,
                                        const float* __restrict__ bias,
                                        float* __restrict__ part,
                                        long long M, int CG) {
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
    sc[j] = weight[c] * is[j];           // folded scale (as in fwd)
    bf[j] = bias[c] - mu[j] * sc[j];     // folded bias
  }
  float8 adb = {0, 0, 0, 0, 0, 0, 0, 0};
  float8 ads = {0, 0, 0, 0, 0, 0, 0, 0};
  auto one = [&](const ushort8& xv, const ushort8& gv) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
      float xf = bf16_to_f32(xv[j]);
      float g = bf16_to_f32(gv[j]);
      if (RELU) {
        // exact fwd replication: y stored as bf16(relu(f))
        float f = fmaf(xf, sc[j], bf[j]);
        if (!f32_to_bf16(f > 0.f ? f : 0.f)) g = 0.f;
      }
      adb[j] += g;
      ads[j] += g * ((xf - mu[j]) * is[j]);
    }
  };
  long long row = rows.first(M);
  for (; row + (KS_BN_UNROLL - 1) * stride < M;
       row += KS_BN_UNROLL * stride) {
    ushort8 xv[KS_BN_UNROLL], gv[KS_BN_UNROLL];
#pragma unroll
    for (int u = 0; u < KS_BN_UNROLL; u++) {
      const long long k = (row + u * stride) * CG + cg;
      xv[u] = x[k];
      gv[u] = dy[k];
    }
#pragma unroll
    for (int u = 0; u < KS_BN_UNROLL; u++) one(xv[u], gv[u]);
  }
  for (; row < M; row += stride) {
    const long long k = row * CG + cg;
    ushort8 xv = x[k], gv = dy[k];
    one(xv, gv);
  }

  const int C = CG * 8;
  nhwc_block_partials<KS_BN_BLOCK>(s_red, adb, part, CG);
  __syncthreads();
  nhwc_block_partials<KS_BN_BLOCK>(s_red, ads,
                                   part + (long long)gridDim.x * C, CG);
}

// ----------------------------------------- bwd apply, no-y variant
template <bool RELU = true>
__global__ void bn_bwd_apply_noy_kernel(const ushort8* __restrict__ x,
                                        const ushort8* __restrict__ dy,
                                        ushort8* __restrict__ dx,
                                        const float* __restrict__ mean,
                                        const float* __restrict__ invstd,
                                        const float* __restrict__ weight,
                                        const float* __restrict__ bias,
                                        const float* __restrict__ dbias,
                                        const float* __restrict__ dscale,
                                        long long M, int CG) {
  const NhwcRows<KS_BN_BLOCK> rows(CG);
  const int cg = rows.cg;
  const long long stride = rows.stride;
  const float invM = 1.f / (float)M;
  float8 mu, is, sc, bf, w, db, ds;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int c = cg * 8 + j;
    mu[j] = mean[c];
    is[j] = invstd[c];
    sc[j] = weight[c] * is[j];
    bf[j] = bias[c] - mu[j] * sc[j];
    w[j] = sc[j];
    db[j] = dbias[c] * invM;
    ds[j] = dscale[c] * invM;
  }
  auto one = [&](const ushort8& xv, const ushort8& gv) {
    ushort8 o;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      float xf = bf16_to_f32(xv[j]);
      float g = bf16_to_f32(gv[j]);
      if (RELU) {
        float f = fmaf(xf, sc[j], bf[j]);
        if (!f32_to_bf16(f > 0.f ? f : 0.f)) g = 0.f;
      }
      float xhat = (xf - mu[j]) * is[j];
      o[j] = f32_to_bf16(w[j] * (g - db[j] - xhat * ds[j]));
    }
    return o;
  };
  long long row = rows.first(M);
  for (; row + (KS_BN_UNROLL - 1) * stride < M;
       row += KS_BN_UNROLL * stride) {
    ushort8 xv[KS_BN_UNROLL], gv[KS_BN_UNROLL];
    long long k[KS_BN_UNROLL];
#pragma unroll
    for (int u = 0; u < KS_BN_UNROLL; u++) {
      k[u] = (row + u * stride) * CG + cg;
      xv[u] = x[k[u]];
      gv[u] = dy[k[u]];
    }
#pragma unroll
    for (int u = 0; u < KS_BN_UNROLL; u++) dx[k[u]] = one(xv[u], gv[u]);
  }
  for (; row < M; row += stride) {
    const long long k = row * CG + cg;
    ushort8 xv = x[k], gv = dy[k];
    dx[k] = one(xv, gv);
  }
}

// ----------------------------------------- bwd apply from dym
// Residual BNs: the stats pass already wrote dym (= dres); read it
// instead of y AND dy — 8 tensor passes -> 7.
__global__ void bn_bwd_apply_dym_kernel(const ushort8* __restrict__ x,
                                        const ushort8* __restrict__ dym,
                                        ushort8* __restrict__ dx,
                                        const float* __restrict__ mean,
                                        const float* __restrict__ invstd,
                                        const float* __restrict__ weight,
                                        const float* __restrict__ dbias,
                                        const float* __restrict__ dscale,
                                        long long M, int CG) {
  const NhwcRows<KS_BN_BLOCK> rows(CG);
  const int cg = rows.cg;
  const long long stride = rows.stride;
  const float invM = 1.f / (float)M;
  float8 mu, is, w, db, ds;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int c = cg * 8 + j;
    mu[j] = mean[c];
    is[j] = invstd[c];
    w[j] = weight[c] * is[j];
    db[j] = dbias[c] * invM;
    ds[j] = dscale[c] * invM;
  }
  // dx = w*invstd * (dym - dbias/M - xhat * dscale/M)
  auto one = [&](const ushort8& xv, const ushort8& gv) {
    ushort8 o;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      float g = bf16_to_f32(gv[j]);  // already ReLU-masked
      float xhat = (bf16_to_f32(xv[j]) - mu[j]) * is[j];
      o[j] = f32_to_bf16(w[j] * (g - db[j] - xhat * ds[j]));
    }
    return o;
  };
  long long row = rows.first(M);
  for (; row + (KS_BN_UNROLL - 1) * stride < M;
       row += KS_BN_UNROLL * stride) {
    ushort8 xv[KS_BN_UNROLL], gv[KS_BN_UNROLL];
    long long k[KS_BN_UNROLL];
#pragma unroll
    for (int u = 0; u < KS_BN_UNROLL; u++) {
      k[u] = (row + u * stride) * CG + cg;
      xv[u] = x[k[u]];
      gv[u] = dym[k[u]];
    }
#pragma unroll
    for (int u = 0; u < KS_BN_UNROLL; u++) dx[k[u]] = one(xv[u], gv[u]);
  }
  for (; row < M; row += stride) {
    const long long k = row * CG + cg;
    ushort8 xv = x[k], gv = dym[k];
    dx[k] = one(xv, gv);
  }
}

// ---------------------------------------------------------- eval apply
__global__ void bn_fold_eval_kernel(const float* __restrict__ weight,
                                    const float* __restrict__ bias,
                                    const float* __restrict__ rmean,
                                    const float* __restrict__ rvar,
                                    float* __restrict__ scale_out,
                                    float* __restrict__ bias_out, int C,
                                    float eps) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float s = weight[c] * rsqrtf(rvar[c] + eps);
  scale_out[c] = s;
  bias_out[c] = bias[c] - rmean[c] * s;
}

// ================================================================ host
void bn_check_mask(const torch::Tensor& mask, const torch::Tensor& x,
                   const BnGeom& g) {
  TORCH_CHECK(mask.is_cuda() && mask.scalar_type() == at::kByte &&
                  mask.is_contiguous() && mask.dim() == 4 &&
                  mask.size(0) == x.size(0) && mask.size(1) == x.size(2) &&
                  mask.size(2) == x.size(3) && mask.size(3) == g.CG,
              "ReLU mask must be a contiguous uint8 (N, H, W, C/8) tensor");
}

BnGeom bn_geom_of(const torch::Tensor& x) {
  TORCH_CHECK(x.dim() == 4, "bn_relu: 4D NCHW tensor expected");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "bn_relu: bf16 only");
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast),
              "bn_relu: channels-last only");
  BnGeom g;
  g.C = (int)x.size(1);
  TORCH_CHECK(g.C % 8 == 0 && g.C <= KS_BN_BLOCK * 8,
              "bn_relu: C must be a multiple of 8 and <= 8*KS_BN_BLOCK");
  g.M = x.numel() / g.C;
  g.CG = g.C / 8;
  long long work = g.M * g.CG;
  long long blocks = (work + KS_BN_BLOCK - 1) / KS_BN_BLOCK;
  // G11: cap + grid-stride (256 CUs want >>256 workgroups)
  g.blocks = (int)std::min<long long>(blocks, 2048);
  g.stat_blocks = (int)std::min<long long>(blocks, 1024);
  if (g.stat_blocks < 1) g.stat_blocks = 1;
  return g;
}

void bn_launch_fwd_stats(const torch::Tensor& x, const BnGeom& g,
                         const torch::Tensor& weight,
                         const torch::Tensor& bias, float* rmean_p,
                         float* rvar_p, torch::Tensor& save_mean,
                         torch::Tensor& save_invstd, torch::Tensor& scale,
                         torch::Tensor& biasf, double momentum, double eps,
                         bool legacy_reduce, hipStream_t stream) {
  auto f32 = x.options().dtype(at::kFloat);
  auto part = at::empty({(long long)2 * g.stat_blocks * g.C}, f32);
  hipLaunchKernelGGL(bn_stats_kernel, dim3(g.stat_blocks),
                     dim3(KS_BN_BLOCK), 0, stream,
                     nhwc_cptr(x),
                     part.data_ptr<float>(), g.M, g.CG);
  if (legacy_reduce) {
    auto sums = at::empty({2 * g.C}, f32);
    hipLaunchKernelGGL(bn_reduce_partials_kernel,
                       dim3((g.C + 3) / 4), dim3(64, 4), 0, stream,
                       part.data_ptr<float>(), g.stat_blocks, g.C,
                       sums.data_ptr<float>(), sums.data_ptr<float>() + g.C);
    int fb = (g.C + 255) / 256;
    hipLaunchKernelGGL(bn_finalize_kernel, dim3(fb), dim3(256), 0,
                       stream, sums.data_ptr<float>(),
                       sums.data_ptr<float>() + g.C,
                       weight.data_ptr<float>(), bias.data_ptr<float>(),
                       rmean_p, rvar_p, save_mean.data_ptr<float>(),
                       save_invstd.data_ptr<float>(),
                       scale.data_ptr<float>(), biasf.data_ptr<float>(), g.M,
                       g.C, (float)momentum, (float)eps);
  } else {
    const BnFinalizeArgs fin = {
        weight.data_ptr<float>(), bias.data_ptr<float>(), rmean_p, rvar_p,
        save_mean.data_ptr<float>(), save_invstd.data_ptr<float>(),
        scale.data_ptr<float>(), biasf.data_ptr<float>(), g.M,
        (float)momentum, (float)eps};
    hipLaunchKernelGGL((bn_reduce_tile_kernel<KS_BN_RTILE, true>),
                       dim3((g.C + KS_BN_RTILE - 1) / KS_BN_RTILE),
                       dim3(64 * KS_BN_RTILE), 0, stream,
                       part.data_ptr<float>(), g.stat_blocks, g.C,
                       (float*)nullptr, (float*)nullptr, fin);
  }
}

void bn_launch_bwd_reduce(const float* part, int nblocks, int C, float* out0,
                          float* out1, bool legacy_reduce,
                          hipStream_t stream) {
  if (legacy_reduce) {
    hipLaunchKernelGGL(bn_reduce_partials_kernel, dim3((C + 3) / 4),
                       dim3(64, 4), 0, stream, part, nblocks, C, out0, out1);
  } else {
    hipLaunchKernelGGL((bn_reduce_tile_kernel<KS_BN_RTILE, false>),
                       dim3((C + KS_BN_RTILE - 1) / KS_BN_RTILE),
                       dim3(64 * KS_BN_RTILE), 0, stream, part, nblocks, C,
                       out0, out1, BnFinalizeArgs{});
  }
}

void bn_launch_reduce_one(const float* part, int nblocks, int C, float* out,
                          hipStream_t stream) {
  hipLaunchKernelGGL((bn_reduce_tile_kernel<KS_BN_RTILE, false, false>),
                     dim3((C + KS_BN_RTILE - 1) / KS_BN_RTILE),
                     dim3(64 * KS_BN_RTILE), 0, stream, part, nblocks, C, out,
                     (float*)nullptr, BnFinalizeArgs{});
}

void bn_launch_fold_eval(const torch::Tensor& weight,
                         const torch::Tensor& bias,
                         const torch::Tensor& rmean,
                         const torch::Tensor& rvar, torch::Tensor& scale,
                         torch::Tensor& biasf, int C, double eps,
                         hipStream_t stream) {
  int fb = (C + 255) / 256;
  hipLaunchKernelGGL(bn_fold_eval_kernel, dim3(fb), dim3(256), 0, stream,
                     weight.data_ptr<float>(), bias.data_ptr<float>(),
                     rmean.data_ptr<float>(), rvar.data_ptr<float>(),
                     scale.data_ptr<float>(), biasf.data_ptr<float>(), C,
                     (float)eps);
}

std::vector<torch::Tensor> bn_relu_fwd_train(
    torch::Tensor x, torch::Tensor weight, torch::Tensor bias,
    torch::Tensor running_mean, torch::Tensor running_var, double momentum,
    double eps, c10::optional<torch::Tensor> res, bool relu,
    bool legacy_reduce, bool want_mask) {
  BnGeom g = bn_geom_of(x);
  TORCH_CHECK(!want_mask || (res.has_value() && relu),
              "bn_relu_fwd_train: the ReLU mask is for residual BNs with "
              "ReLU");
  auto stream = at::cuda::getCurrentCUDAStream();
  auto f32 = x.options().dtype(at::kFloat);
  auto y = at::empty_like(x);
  // one byte per lane and row: (N, H, W, C/8)
  torch::Tensor mask;
  if (want_mask)
    mask = at::empty({x.size(0), x.size(2), x.size(3), (long long)g.CG},
                     x.options().dtype(at::kByte));
  auto save_mean = at::empty({g.C}, f32);
  auto save_invstd = at::empty({g.C}, f32);
  auto scale = at::empty({g.C}, f32);
  auto biasf = at::empty({g.C}, f32);
  float* rmean_p =
      running_mean.defined() ? running_mean.data_ptr<float>() : nullptr;
  float* rvar_p =
      running_var.defined() ? running_var.data_ptr<float>() : nullptr;
  bn_launch_fwd_stats(x, g, weight, bias, rmean_p, rvar_p, save_mean,
                      save_invstd, scale, biasf, momentum, eps, legacy_reduce,
                      stream.stream());
  auto launch_apply = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(g.blocks), dim3(KS_BN_BLOCK), 0,
                       stream.stream(),
                       nhwc_cptr(x),
                       res.has_value()
                           ? nhwc_cptr(*res)
                           : nullptr,
                       nhwc_mptr(y),
                       want_mask ? mask.data_ptr<unsigned char>() : nullptr,
                       scale.data_ptr<float>(), biasf.data_ptr<float>(), g.M,
                       g.CG);
  };
  if (want_mask)
    launch_apply(bn_apply_relu_kernel<true, true, true>);
  else if (res.has_value())
    relu ? launch_apply(bn_apply_relu_kernel<true, true>)
         : launch_apply(bn_apply_relu_kernel<true, false>);
  else
    relu ? launch_apply(bn_apply_relu_kernel<false, true>)
         : launch_apply(bn_apply_relu_kernel<false, false>);
  if (want_mask) return {y, save_mean, save_invstd, mask};
  return {y, save_mean, save_invstd};
}

torch::Tensor bn_relu_fwd_eval(torch::Tensor x, torch::Tensor weight,
                               torch::Tensor bias, torch::Tensor rmean,
                               torch::Tensor rvar, double eps,
                               c10::optional<torch::Tensor> res, bool relu) {
  BnGeom g = bn_geom_of(x);
  auto stream = at::cuda::getCurrentCUDAStream();
  auto f32 = x.options().dtype(at::kFloat);
  auto scale = at::empty({g.C}, f32);
  auto biasf = at::empty({g.C}, f32);
  auto y = at::empty_like(x);
  bn_launch_fold_eval(weight, bias, rmean, rvar, scale, biasf, g.C, eps,
                      stream.stream());
  auto launch_apply = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(g.blocks), dim3(KS_BN_BLOCK), 0,
                       stream.stream(),
                       nhwc_cptr(x),
                       res.has_value()
                           ? nhwc_cptr(*res)
                           : nullptr,
                       nhwc_mptr(y),
                       (unsigned char*)nullptr, scale.data_ptr<float>(),
                       biasf.data_ptr<float>(), g.M, g.CG);
  };
  if (res.has_value())
    relu ? launch_apply(bn_apply_relu_kernel<true, true>)
         : launch_apply(bn_apply_relu_kernel<true, false>);
  else
    relu ? launch_apply(bn_apply_relu_kernel<false, true>)
         : launch_apply(bn_apply_relu_kernel<false, false>);
  return y;
}

std::vector<torch::Tensor> bn_relu_bwd(
    torch::Tensor x, c10::optional<torch::Tensor> y, torch::Tensor dy,
    torch::Tensor weight, torch::Tensor bias, torch::Tensor mean,
    torch::Tensor invstd, bool need_dres, bool relu,
    c10::optional<torch::Tensor> dy2, bool legacy_reduce,
    c10::optional<torch::Tensor> mask) {
  TORCH_CHECK(relu || !need_dres,
              "bn_relu_bwd: residual path requires the ReLU variant");
  BnGeom g = bn_geom_of(x);
  TORCH_CHECK(dy.sizes() == x.sizes() && dy.scalar_type() == at::kBFloat16,
              "bn_relu_bwd: dy must be bf16 of x's shape");
  // residual BNs take the ReLU mask from y, or from the byte mask the
  // forward left (bn_apply_relu_kernel<.., MASK>) when that is given
  const bool use_mask = need_dres && mask.has_value() && mask->defined();
  if (use_mask) {
    bn_check_mask(*mask, x, g);
  } else if (need_dres) {
    TORCH_CHECK(y.has_value() && y->defined() && y->sizes() == x.sizes() &&
                    y->scalar_type() == at::kBFloat16 &&
                    y->is_contiguous(at::MemoryFormat::ChannelsLast),
                "bn_relu_bwd: y must be channels-last bf16 of x's shape");
  }
  // second upstream gradient (y forked to two consumers): folded into
  // the residual stats kernel when it has dy's layout; anything else is
  // summed here first and takes the existing path
  bool fold_dy2 = false;
  if (dy2.has_value() && dy2->defined()) {
    TORCH_CHECK(dy2->sizes() == x.sizes(),
                "bn_relu_bwd: dy2 must have x's shape");
    fold_dy2 = need_dres && dy2->is_cuda() &&
               dy2->scalar_type() == at::kBFloat16 &&
               dy2->is_contiguous(at::MemoryFormat::ChannelsLast) &&
               dy.is_contiguous(at::MemoryFormat::ChannelsLast);
    if (!fold_dy2) dy = (dy + *dy2).to(at::kBFloat16);
  }
  auto stream = at::cuda::getCurrentCUDAStream();
  auto f32 = x.options().dtype(at::kFloat);
  auto part = at::empty({(long long)2 * g.stat_blocks * g.C}, f32);
  auto red = at::empty({g.C * 2}, f32);
  float* dbias_p = red.data_ptr<float>();
  float* dscale_p = dbias_p + g.C;
  auto dx = at::empty_like(x);
  torch::Tensor dres;
  if (!dy.is_contiguous(at::MemoryFormat::ChannelsLast))
    dy = dy.contiguous(at::MemoryFormat::ChannelsLast);
  // block partials -> dbias, dscale
  auto launch_reduce = [&]() {
    bn_launch_bwd_reduce(part.data_ptr<float>(), g.stat_blocks, g.C, dbias_p,
                         dscale_p, legacy_reduce, stream.stream());
  };

  if (need_dres) {
    // residual: the stats pass writes dym (= dres), the apply pass
    // reads it back instead of y AND dy (8 tensor passes -> 7)
    dres = at::empty_like(x);
    auto launch_rstats = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3(g.stat_blocks), dim3(KS_BN_BLOCK), 0,
                         stream.stream(),
                         nhwc_cptr(x),
                         use_mask ? nullptr
                                  : nhwc_cptr(*y),
                         use_mask ? mask->data_ptr<unsigned char>() : nullptr,
                         nhwc_cptr(dy),
                         fold_dy2 ? nhwc_cptr(*dy2)
                                  : nullptr,
                         nhwc_mptr(dres),
                         mean.data_ptr<float>(), invstd.data_ptr<float>(),
                         part.data_ptr<float>(), g.M, g.CG);
    };
    if (use_mask)
      fold_dy2 ? launch_rstats(bn_bwd_stats_kernel<true, true, true>)
               : launch_rstats(bn_bwd_stats_kernel<true, false, true>);
    else
      fold_dy2 ? launch_rstats(bn_bwd_stats_kernel<true, true>)
               : launch_rstats(bn_bwd_stats_kernel<true, false>);
    launch_reduce();
    hipLaunchKernelGGL(bn_bwd_apply_dym_kernel, dim3(g.blocks),
                       dim3(KS_BN_BLOCK), 0, stream.stream(),
                       nhwc_cptr(x),
                       nhwc_cptr(dres),
                       nhwc_mptr(dx),
                       mean.data_ptr<float>(), invstd.data_ptr<float>(),
                       weight.data_ptr<float>(), dbias_p, dscale_p,
                       g.M, g.CG);
    auto dbias = red.narrow(0, 0, g.C);
    auto dscale = red.narrow(0, g.C, g.C);
    return {dx, dscale, dbias, dres};
  }
  // non-residual: the ReLU mask is recomputed from x and the folded
  // scale/bias, so y is never read (7 tensor passes -> 5)
  auto launch_stats = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(g.stat_blocks), dim3(KS_BN_BLOCK), 0,
                       stream.stream(),
                       nhwc_cptr(x),
                       nhwc_cptr(dy),
                       mean.data_ptr<float>(), invstd.data_ptr<float>(),
                       weight.data_ptr<float>(), bias.data_ptr<float>(),
                       part.data_ptr<float>(), g.M, g.CG);
  };
  relu ? launch_stats(bn_bwd_stats_noy_kernel<true>)
       : launch_stats(bn_bwd_stats_noy_kernel<false>);
  launch_reduce();
  auto launch_bapply = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(g.blocks), dim3(KS_BN_BLOCK), 0,
                       stream.stream(),
                       nhwc_cptr(x),
                       nhwc_cptr(dy),
                       nhwc_mptr(dx),
                       mean.data_ptr<float>(), invstd.data_ptr<float>(),
                       weight.data_ptr<float>(), bias.data_ptr<float>(),
                       dbias_p, dscale_p, g.M, g.CG);
  };
  relu ? launch_bapply(bn_bwd_apply_noy_kernel<true>)
       : launch_bapply(bn_bwd_apply_noy_kernel<false>);
  auto dbias = red.narrow(0, 0, g.C);
  auto dscale = red.narrow(0, g.C, g.C);
  return {dx, dscale, dbias};
}
