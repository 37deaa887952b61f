// What every fused NHWC bf16 kernel of this extension shares (bn_relu,
// bn_join, bn_pool, bias_relu, pool): the vector types, the bf16
// conversions, how a block walks the rows of an activation and how it
// leaves per-channel partial sums. Each convention is explained here,
// once; the .hip files refer to it.
//
// Layout: channels-last bf16 with C % 8 == 0. A "row" is one pixel
// (n, h, w), M = N*H*W of them; one lane owns 8 CONSECUTIVE channels of
// a row (one 16-byte access), so a row takes CG = C/8 lanes,
// per-channel reductions never cross lanes and a wave's 64 lanes cover
// 1 KiB of contiguous memory. Element offsets (row * CG + cg, in units
// of 8 channels) are 64-bit: VGG16's first pool at batch 256 is 822 M
// elements. Pixel indices are 32-bit where a kernel decomposes them into
// (n, h, w); the host checks N*H*W < 2**31 there.
//
// (cast_common.h's conversion canonicalises NaNs and stays separate:
// f32_to_bf16 here deliberately does not.)
#pragma once
#include <hip/hip_runtime.h>
#include <torch/extension.h>

typedef __attribute__((ext_vector_type(8))) unsigned short ushort8;
typedef __attribute__((ext_vector_type(8))) float float8;

__device__ __forceinline__ float bf16_to_f32(unsigned short u) {
  union {
    unsigned int i;
    float f;
  } v;
  v.i = ((unsigned int)u) << 16;
  return v.f;
}

__device__ __forceinline__ unsigned short f32_to_bf16(float f) {
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

// ---------------------------------------------------------------- row walk
// Thread tid of a BLOCK-thread block owns channel group cg = tid % CG of
// the block's row tid / CG, so a block holds BLOCK / CG rows. When CG
// does not divide BLOCK the tail threads (tid / CG >= BLOCK / CG) would
// alias the NEXT block's rows: they must idle. Here they start at row M,
// so every loop over rows is empty for them, they still reach every
// __syncthreads() and their accumulators stay zero.
//
// Grid-stride form: a lane visits first, first + stride, ... < M. The
// kernels advance in groups of KS_BN_UNROLL rows while a whole group
// fits and finish row by row; which rows a lane visits, in which order
// and in which groups is part of the numerical contract of the kernels
// that sum over rows (bn_common.h, bn_acc_dscale).
template <int BLOCK>
class NhwcRows {
 public:
  int cg;            // channel group of this lane
  long long stride;  // rows between two visits of a lane

  __device__ __forceinline__ explicit NhwcRows(int CG) {
    const int tid = threadIdx.x;
    cg = tid % CG;
    roff = tid / CG;
    rows_per_blk = BLOCK / CG;
    active = roff < rows_per_blk;
    stride = (long long)gridDim.x * rows_per_blk;
  }
  // first row of this lane, M for an idle one; kernels call it where
  // their row loop starts
  __device__ __forceinline__ long long first(long long M) const {
    return active ? (long long)blockIdx.x * rows_per_blk + roff : M;
  }

 private:
  int roff, rows_per_blk;  // row of this lane within the block, of how many
  bool active;             // false for the idle tail threads
};

// Single-row form (the pool kernels: one lane, one pixel, no loop and no
// barrier afterwards): false for an idle tail thread and past the last
// row, otherwise the lane's channel group and its 32-bit pixel index.
template <int BLOCK>
__device__ __forceinline__ bool nhwc_one_row(int M, int CG, int& cg,
                                             int& row) {
  const int tid = threadIdx.x;
  cg = tid % CG;
  const int roff = tid / CG;
  const int rows_per_blk = BLOCK / CG;
  if (roff >= rows_per_blk) return false;
  const long long row64 = (long long)blockIdx.x * rows_per_blk + roff;
  if (row64 >= M) return false;
  row = (int)row64;
  return true;
}

// ---------------------------------------------------------- block partials
// Sum of `acc` over the lanes of a block that share a channel group: an
// LDS tree (s_red holds BLOCK * 8 floats; lane tid < CG adds the rows
// r = 0, 1, ... of its group in ascending order), then plain stores to
// the block's row of part[blocks][C], which a reduce kernel sums
// afterwards. No atomics: the order is fixed. Every thread of the block
// calls it, idle tail threads with zeros; two calls that share s_red
// need a __syncthreads() between them.
template <int BLOCK>
__device__ __forceinline__ void nhwc_block_partials(
    float* __restrict__ s_red, const float8& acc, float* __restrict__ part,
    int CG) {
  const int tid = threadIdx.x;
  const int rows_per_blk = BLOCK / CG;
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

// ------------------------------------------------------------------ host
// A bf16 tensor's storage as vectors of 8 channels.
inline const ushort8* nhwc_cptr(const torch::Tensor& t) {
  return reinterpret_cast<const ushort8*>(t.data_ptr());
}

inline ushort8* nhwc_mptr(const torch::Tensor& t) {
  return reinterpret_cast<ushort8*>(t.data_ptr());
}
