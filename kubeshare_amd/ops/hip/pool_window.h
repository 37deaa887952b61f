// The max-pool window code shared by pool.hip, bn_pool.hip and
// bias_relu.hip: the forward scan with its one-byte argmax codes, the
// backward gather that reads them, and the host-side geometry with the
// checks every pooled op makes on its input (declared here, defined once
// in pool.hip, as bn_geom_of lives in bn_relu.hip). Layout conventions
// and the one-row prologue are nhwc_common.h's.
//
// Forward rule (PyTorch's, row-major over the in-bounds positions of a
// K x K window):  if (val > maxval || isnan(val)) take it,
// starting from maxval = -inf. The forward stores, per output element,
// the window-local position kh*K + kw of the winner in ONE byte; eight
// of them (a lane's channels) make a uint2. The backward is a gather
// over input pixels: every input element is written exactly once, so
// there is no memset of dx, there are no atomics and the result is
// deterministic.
#pragma once
#include "nhwc_common.h"

// --------------------------------------------------------------- forward
// One lane = 8 channels of one OUTPUT pixel. load() issues the K*K loads
// at CLAMPED (always in-bounds) addresses, so they are unconditional and
// all in flight before the first compare; positions that fall into the
// padding are masked out of the scan instead. A kernel loads its
// per-channel constants between load() and scan().
template <int K, int S>
struct PoolWindow {
  ushort8 v[K * K];
  bool ok[K * K];
  unsigned int q0;  // first in-bounds position (pad < K: there is one)

  // row = output pixel (n, oh, ow) < N*OH*OW
  __device__ __forceinline__ void load(const ushort8* __restrict__ x, int row,
                                       int H, int W, int OH, int OW, int pad,
                                       int CG, int cg) {
    const int ow = row % OW;
    const int t = row / OW;
    const int oh = t % OH;
    const int n = t / OH;
    const int h0 = oh * S - pad;
    const int w0 = ow * S - pad;
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
    q0 = (unsigned int)((h0 < 0 ? -h0 : 0) * K + (w0 < 0 ? -w0 : 0));
  }

  // The scan over map(bits, j), the bf16 bits channel j of a loaded
  // value stands for (identity for the plain pool; a fused op passes the
  // value its unpooled kernel would have stored, rounded to bf16 BEFORE
  // comparing). Returns the winners' bits (the max of bf16 values is
  // exact) and leaves their window positions in `code`; a kernel that
  // stores them packs them with pool_pack_codes.
  template <typename Map>
  __device__ __forceinline__ ushort8 scan(Map map,
                                          unsigned int (&code)[8]) const {
    float best[8];
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
          const unsigned short yb = map(v[q][j], j);
          const float f = bf16_to_f32(yb);
          if (f > best[j] || f != f) {
            best[j] = f;
            o[j] = yb;
            code[j] = q;
          }
        }
      }
    }
    return o;
  }
};

// A lane's eight one-byte codes as the uint2 the forward stores.
__device__ __forceinline__ uint2 pool_pack_codes(
    const unsigned int (&code)[8]) {
  uint2 c;
  c.x = code[0] | (code[1] << 8) | (code[2] << 16) | (code[3] << 24);
  c.y = code[4] | (code[5] << 8) | (code[6] << 16) | (code[7] << 24);
  return c;
}

// -------------------------------------------------------------- backward
// What one lane needs to form the pool gradient of 8 channels of one
// INPUT pixel (n, h, w), kept apart from the arithmetic so that a
// sub-batch of rows can issue all its loads first. The windows that
// cover the pixel are oh in [ceil((h+pad-K+1)/S), floor((h+pad)/S)]
// clamped to [0, OH) (same for ow): at most NW = ceil(K/S) per axis,
// visited in ascending (oh, ow) order. dy is added where the stored code
// equals this pixel's position inside that window; f32 accumulation, one
// RNE rounding, zero if nothing selected the pixel.
// WITH_Y (bias_relu.hip): also loads the pooled y of each window and
// adds only where it is > 0, the ReLU mask of the selected element.
template <int K, int S, bool WITH_Y = false>
struct PoolGather {
  static constexpr int NW = (K + S - 1) / S;
  ushort8 g[NW * NW];
  ushort8 yv[WITH_Y ? NW * NW : 1];
  uint2 c[NW * NW];
  unsigned int want[NW * NW];
  bool ok[NW * NW];

  // row = input pixel < N*H*W; y is read only WITH_Y
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
      // not exist (OH >= 1 always; oh_lo >= 0, and the clamp covers every
      // oh >= OH)
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
        if (WITH_Y) yv[q] = y[k];
        c[q] = idx[k];
      }
    }
  }

  // channel j's gradient as bf16 bits, the value an unfused pool
  // backward stores
  __device__ __forceinline__ unsigned short grad_bits(int j) const {
    float acc = 0.f;
#pragma unroll
    for (int q = 0; q < NW * NW; q++) {
      if (ok[q]) {
        const unsigned int word = j < 4 ? c[q].x : c[q].y;
        const unsigned int code = (word >> (8 * (j & 3))) & 0xffu;
        if (code == want[q] &&
            (!WITH_Y || bf16_to_f32(yv[WITH_Y ? q : 0][j]) > 0.f))
          acc += bf16_to_f32(g[q][j]);
      }
    }
    return f32_to_bf16(acc);
  }

  // the same value widened again, as a kernel reading that store sees it
  __device__ __forceinline__ float grad(int j) const {
    return bf16_to_f32(grad_bits(j));
  }
};

// ------------------------------------------------------------------ host
// threads of a pooled forward block: one lane = 8 channels of one output
// pixel, one block spans at least one pixel's channel groups
#define KS_POOL_BLOCK 256

struct PoolGeom {
  int N, C, H, W, OH, OW, CG, pad;
  long long MO;  // output pixels
};

// (k, s, p) must be one of the compiled configurations, (3, 2, 1) or
// (2, 2, 0).
void pool_check_cfg(const char* op, int64_t k, int64_t s, int64_t p);

// For a checked (k, s, p): C a multiple of 8 in [8, 8*KS_POOL_BLOCK], a
// non-empty output, N*H*W < 2**31 (pixel indices are 32-bit); then the
// output size.
PoolGeom pool_geom(const char* op, int64_t N, int64_t C, int64_t H, int64_t W,
                   int64_t k, int64_t s, int64_t p);

// Blocks of KS_POOL_BLOCK threads for M rows of CG lanes each.
inline unsigned int pool_blocks_for(long long M, int CG) {
  const int rows_per_blk = KS_POOL_BLOCK / CG;
  return (unsigned int)((M + rows_per_blk - 1) / rows_per_blk);
}
