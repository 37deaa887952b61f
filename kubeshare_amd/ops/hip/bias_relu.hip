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
// Conventions are bn_relu.hip's and pool.hip's: channels-last bf16,
// C % 8 == 0, one lane owns 8 CONSECUTIVE channels (one 16-byte access),
// 64-bit element offsets, 32-bit pixel indices (the host checks
// N*H*W < 2**31), f32 arithmetic, tail threads idle when C/8 does not
// divide the block. No atomics: every result is a fixed-order sum.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <vector>

#include "bn_common.h"

#define KS_BR_POOL_BLOCK 256  // pool.hip's KS_POOL_BLOCK
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

// LDS tree over the lanes sharing a channel group (bn_stats_kernel's),
// then plain stores of the block's row of `part`. Every thread of the
// block calls it (idle tail threads with zeros).
__device__ __forceinline__ void bias_relu_block_partials(
    float* __restrict__ s_red, const float8& acc, float* __restrict__ part,
    int CG) {
  const int tid = threadIdx.x;
  const int rows_per_blk = KS_BN_BLOCK / CG;
#pragma unroll
  for (int j = 0; j < 8; j++) s_red[tid * 8 + j] = acc[j];
  __syncthreads();
  if (tid < CG) {
    float8 t = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int r = 0; r < rows_per_blk; r++)
#pragma unroll
      for (int j = 0; j < 8; j++) t[j] += s_red[(r * CG + tid) * 8 + j];
    float* row = part + (long long)blockIdx.x * (CG * 8);
#pragma unroll
    for (int j = 0; j < 8; j++) row[tid * 8 + j] = t[j];
  }
}

// --------------------------------------------------------------- forward
__global__ void __launch_bounds__(KS_BN_BLOCK)
bias_relu_fwd_kernel(const ushort8* __restrict__ x, ushort8* __restrict__ y,
                     const float* __restrict__ bias, long long M, int CG) {
  const int tid = threadIdx.x;
  const int cg = tid % CG;
  const int roff = tid / CG;
  const int rows_per_blk = KS_BN_BLOCK / CG;
  const bool active = roff < rows_per_blk;  // see bn_stats_kernel
  const long long stride = (long long)gridDim.x * rows_per_blk;
  float8 b;
#pragma unroll
  for (int j = 0; j < 8; j++) b[j] = bias[cg * 8 + j];
  long long row = active ? (long long)blockIdx.x * rows_per_blk + roff : M;
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
    for (int u = 0; u < KS_BN_UNROLL; u++) {
      ushort8 o;
#pragma unroll
      for (int j = 0; j < 8; j++) o[j] = bias_relu_bf16(v[u][j], b[j]);
      y[k[u]] = o;
    }
  }
  for (; row < M; row += stride) {
    const long long k = row * CG + cg;
    const ushort8 v = x[k];
    ushort8 o;
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = bias_relu_bf16(v[j], b[j]);
    y[k] = o;
  }
}

// -------------------------------------------------------------- backward
// dx = y > 0 ? dy : 0, db partials: part[b*C + c].
__global__ void __launch_bounds__(KS_BN_BLOCK)
bias_relu_bwd_kernel(const ushort8* __restrict__ dy,
                     const ushort8* __restrict__ y, ushort8* __restrict__ dx,
                     float* __restrict__ part, long long M, int CG) {
  __shared__ float s_red[KS_BN_BLOCK * 8];
  const int tid = threadIdx.x;
  const int cg = tid % CG;
  const int roff = tid / CG;
  const int rows_per_blk = KS_BN_BLOCK / CG;
  const bool active = roff < rows_per_blk;  // see bn_stats_kernel
  const long long stride = (long long)gridDim.x * rows_per_blk;
  float8 adb = {0, 0, 0, 0, 0, 0, 0, 0};
  long long row = active ? (long long)blockIdx.x * rows_per_blk + roff : M;
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
    for (int u = 0; u < KS_BN_UNROLL; u++) {
      ushort8 o;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        o[j] = bf16_to_f32(yv[u][j]) > 0.f ? gv[u][j] : (unsigned short)0;
        adb[j] += bf16_to_f32(o[j]);
      }
      dx[k[u]] = o;
    }
  }
  for (; row < M; row += stride) {
    const long long k = row * CG + cg;
    const ushort8 gv = dy[k], yv = y[k];
    ushort8 o;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      o[j] = bf16_to_f32(yv[j]) > 0.f ? gv[j] : (unsigned short)0;
      adb[j] += bf16_to_f32(o[j]);
    }
    dx[k] = o;
  }
  bias_relu_block_partials(s_red, adb, part, CG);
}

// -------------------------------------------------------- pooled forward
// max_pool_nhwc_fwd_kernel with the bias + ReLU applied to every loaded
// value. Rule (pool.hip's): start from -inf at the first in-bounds
// position, take a value if val > best || isnan(val), row-major.
template <int K, int S, bool WANT_IDX>
__global__ void __launch_bounds__(KS_BR_POOL_BLOCK)
bias_relu_pool_fwd_kernel(const ushort8* __restrict__ x,
                          ushort8* __restrict__ y, uint2* __restrict__ idx,
                          const float* __restrict__ bias, int H, int W,
                          int OH, int OW, int pad, int M, int CG) {
  const int tid = threadIdx.x;
  const int cg = tid % CG;
  const int roff = tid / CG;
  const int rows_per_blk = KS_BR_POOL_BLOCK / CG;
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
  float8 b;
#pragma unroll
  for (int j = 0; j < 8; j++) b[j] = bias[cg * 8 + j];

  // first in-bounds position of the window (pad < K: there is one)
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
        // the value bias_relu_fwd_kernel would have stored
        const unsigned short yb = bias_relu_bf16(v[q][j], b[j]);
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

// ------------------------------------------------------- pooled backward
// What one lane needs for 8 channels of one input pixel:
// max_pool_nhwc_bwd_kernel's loads and bookkeeping plus the pooled y of
// each covering window, kept apart from the arithmetic so that a
// sub-batch can issue all its loads first.
template <int K, int S>
struct BiasReluPoolGather {
  static constexpr int NW = (K + S - 1) / S;
  ushort8 g[NW * NW];
  ushort8 yv[NW * NW];
  uint2 c[NW * NW];
  unsigned int want[NW * NW];
  bool ok[NW * NW];

  // row = input pixel (n, h, w) < N*H*W
  __device__ __forceinline__ void load(const ushort8* __restrict__ dy,
                                       const uint2* __restrict__ idx,
                                       const ushort8* __restrict__ y, int row,
                                       int H, int W, int OH, int OW, int pad,
                                       int CG, int cg) {
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
      // not exist (OH >= 1 always; oh_lo <= h + pad < H + pad, and the
      // clamp below covers every oh >= OH)
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
        yv[q] = y[k];
        c[q] = idx[k];
      }
    }
  }

  // channel j's dx: covering windows in ascending (oh, ow) order, dy
  // added where the stored code is this pixel's position and the pooled
  // y is positive; f32 sum, one RNE rounding
  __device__ __forceinline__ unsigned short grad(int j) const {
    float acc = 0.f;
#pragma unroll
    for (int q = 0; q < NW * NW; q++) {
      if (ok[q]) {
        const unsigned int word = j < 4 ? c[q].x : c[q].y;
        const unsigned int code = (word >> (8 * (j & 3))) & 0xffu;
        if (code == want[q] && bf16_to_f32(yv[q][j]) > 0.f)
          acc += bf16_to_f32(g[q][j]);
      }
    }
    return f32_to_bf16(acc);
  }
};

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
  const int tid = threadIdx.x;
  const int cg = tid % CG;
  const int roff = tid / CG;
  const int rows_per_blk = KS_BN_BLOCK / CG;
  const bool active = roff < rows_per_blk;  // see bn_stats_kernel
  const long long stride = (long long)gridDim.x * rows_per_blk;
  float8 adb = {0, 0, 0, 0, 0, 0, 0, 0};
  long long row = active ? (long long)blockIdx.x * rows_per_blk + roff : M;
  for (; row + (KS_BN_UNROLL - 1) * stride < M;
       row += KS_BN_UNROLL * stride) {
    // a real loop: unrolled, the next sub-batch's loads are hoisted over
    // this one's arithmetic and the registers run out
#pragma unroll 1
    for (int h = 0; h < KS_BN_UNROLL; h += U) {
      long long k[U];
      BiasReluPoolGather<K, S> pg[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const long long r = row + (h + u) * stride;
        k[u] = r * CG + cg;
        pg[u].load(dy, idx, y, (int)r, H, W, OH, OW, pad, CG, cg);
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        ushort8 o;
#pragma unroll
        for (int j = 0; j < 8; j++) {
          o[j] = pg[u].grad(j);
          adb[j] += bf16_to_f32(o[j]);
        }
        dx[k[u]] = o;
      }
    }
  }
  for (; row < M; row += stride) {
    BiasReluPoolGather<K, S> pg;
    pg.load(dy, idx, y, (int)row, H, W, OH, OW, pad, CG, cg);
    ushort8 o;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      o[j] = pg.grad(j);
      adb[j] += bf16_to_f32(o[j]);
    }
    dx[row * CG + cg] = o;
  }
  bias_relu_block_partials(s_red, adb, part, CG);
}

// ================================================================== host
namespace {

void check_cfg(int64_t k, int64_t s, int64_t p) {
  TORCH_CHECK((k == 3 && s == 2 && p == 1) || (k == 2 && s == 2 && p == 0),
              "bias_relu_pool: (k, s, p) must be (3, 2, 1) or (2, 2, 0)");
}

// x-shaped tensor of either op: 4-D bf16 channels-last on the GPU,
// C % 8 == 0, 8 <= C <= 2048, at least one pixel, N*H*W < 2**31
BnGeom geom_of(const torch::Tensor& x, const char* what) {
  TORCH_CHECK(x.is_cuda(), what, ": GPU tensor expected");
  BnGeom g = bn_geom_of(x);  // dim, dtype, layout, C % 8
  TORCH_CHECK(g.C >= 8 && g.C <= KS_BR_POOL_BLOCK * 8, what,
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

struct PoolOut {
  int OH, OW;
};

PoolOut pool_out(int64_t H, int64_t W, int64_t k, int64_t s, int64_t p) {
  TORCH_CHECK(H + 2 * p >= k && W + 2 * p >= k,
              "bias_relu_pool: empty output");
  PoolOut o;
  o.OH = (int)((H + 2 * p - k) / s + 1);
  o.OW = (int)((W + 2 * p - k) / s + 1);
  return o;
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
                     reinterpret_cast<const ushort8*>(x.data_ptr()),
                     reinterpret_cast<ushort8*>(y.data_ptr()),
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
                     reinterpret_cast<const ushort8*>(dy.data_ptr()),
                     reinterpret_cast<const ushort8*>(y.data_ptr()),
                     reinterpret_cast<ushort8*>(dx.data_ptr()),
                     part.data_ptr<float>(), g.M, g.CG);
  return {dx, reduce_db(part, g, stream.stream())};
}

// Returns {y} or, with want_idx, {y, idx}: y (N, C, OH, OW) bf16
// channels-last, idx (N, OH, OW, C) uint8 window codes.
std::vector<torch::Tensor> bias_relu_pool_fwd(torch::Tensor x,
                                              torch::Tensor bias, int64_t k,
                                              int64_t s, int64_t p,
                                              bool want_idx) {
  check_cfg(k, s, p);
  BnGeom g = geom_of(x, "bias_relu_pool_fwd");
  check_bias(g, bias, "bias_relu_pool_fwd");
  const int N = (int)x.size(0), H = (int)x.size(2), W = (int)x.size(3);
  const PoolOut o = pool_out(H, W, k, s, p);
  auto stream = at::cuda::getCurrentCUDAStream();
  auto y = at::empty({N, g.C, o.OH, o.OW},
                     x.options().memory_format(at::MemoryFormat::ChannelsLast));
  torch::Tensor idx;
  if (want_idx)
    idx = at::empty({N, o.OH, o.OW, g.C}, x.options().dtype(at::kByte));
  const long long MO = (long long)N * o.OH * o.OW;  // <= N*H*W < 2**31
  const int rows_per_blk = KS_BR_POOL_BLOCK / g.CG;
  const unsigned int blocks =
      (unsigned int)((MO + rows_per_blk - 1) / rows_per_blk);
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(KS_BR_POOL_BLOCK), 0,
                       stream.stream(),
                       reinterpret_cast<const ushort8*>(x.data_ptr()),
                       reinterpret_cast<ushort8*>(y.data_ptr()),
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
  check_cfg(k, s, p);
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
  const int N = (int)input_sizes[0], H = (int)input_sizes[2],
            W = (int)input_sizes[3];
  const PoolOut o = pool_out(H, W, k, s, p);
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
                       reinterpret_cast<const ushort8*>(dy.data_ptr()),
                       reinterpret_cast<const uint2*>(idx.data_ptr()),
                       reinterpret_cast<const ushort8*>(y.data_ptr()),
                       reinterpret_cast<ushort8*>(dx.data_ptr()),
                       part.data_ptr<float>(), H, W, o.OH, o.OW, (int)p, g.M,
                       g.CG);
  };
  if (k == 3)
    launch(bias_relu_pool_bwd_kernel<3, 2, KS_BR_U_321>);
  else
    launch(bias_relu_pool_bwd_kernel<2, 2, KS_BR_U_220>);
  return {dx, reduce_db(part, g, stream.stream())};
}
