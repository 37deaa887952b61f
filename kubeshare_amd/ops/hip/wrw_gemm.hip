// wrw_gemm_1x1: the weight gradient of a stride-1 1x1 convolution as a
// deterministic split-K bf16 MFMA GEMM for gfx950 (CDNA4, wave64).
//
// With channels-last activations X is [P, C] and dY is [P, K], P = N*H*W,
// and dW[k, c] = sum_p dY[p, k] * X[p, c]: a GEMM whose reduction runs
// over the pixels, the strided dimension of both operands in memory.
//
// Two kernels, no atomics ("1x1 weight gradients as a split-K
// MFMA GEMM"):
//  - wrw_gemm_kernel: grid (output tiles) x (S pixel slices). A block of
//    four waves owns a TM x TN tile of dW (TM rows of K, TN columns of C;
//    256x64, 64x256 or 128x128, every wave a 64x64 sub-tile of 2x2
//    v_mfma_f32_32x32x16_bf16 accumulators) and walks its slice in tiles
//    of 32 pixels. It writes its f32 partial tile to the workspace
//    [S][K][C], or, when S == 1, rounds to bf16 and writes dW itself.
//  - wrw_reduce_kernel: dW = bf16(sum over s of the partials), added in
//    a fixed order (16 runs of consecutive slices, each in slice order,
//    then the runs in order), rounded once.
// Tile shape, S and the slice length are a pure function of (P, C, K)
// (wrw_plan): nothing is asked of the device, so the same inputs give the
// same bits on every run.
//
// Data movement. A 16-byte global load brings 8 channels of one pixel; the
// MFMA wants from each lane 8 pixels of one channel. A loading thread
// therefore takes a unit of 8 channels x 8 pixels (eight 16-byte loads, a
// pixel each, neighbouring lanes on neighbouring channel groups of the
// same pixel), transposes the 8x8 block of 16-bit values in registers and
// writes eight 16-byte LDS rows, channel-major: LDS holds [channel][32
// pixels] with rows of 80 bytes (64 + 16 of padding, which spreads the 16
// lanes of a 128-bit read pass over all 64 banks). A lane's A or B
// operand is then one ds_read_b128. The loads of pixel tile t+1 are issued
// before the MFMAs of tile t and written to the other LDS buffer after
// them: one barrier per tile.
//
// Edges. Channel groups beyond K or C and pixels beyond the slice are
// loaded as zeros (C % 8 == 0 and K % 8 == 0, so a group is in or out as a
// whole); the MFMA loop has no branches, and the epilogue masks its
// stores. Byte offsets are 64-bit.
//
// wrw_gemm_conv: the same engine as an implicit GEMM for 3x3 kernels and
// stride 2 ("3x3 and stride-2 weight gradients on the same
// engine"). With Q = N*Ho*Wo output pixels,
//   dW[k, r, s, c] = sum_q dY[q, k] * X[n, ho*st + r - p, wo*st + s - p, c]
// where a position outside the image counts as zero. wrw_conv_kernel is
// the kernel above with two changes:
//  - the B operand is gathered. A unit is still 8 channels x 8 pixels,
//    but the pixels are consecutive OUTPUT pixels of one tap (r, s): the
//    thread keeps (n, ho, wo) of its first pixel (divided out once, when
//    the slice starts, then moved 32 pixels per tile with carries), walks
//    the other seven with carries, and builds an 8-bit mask of the pixels
//    that are inside the slice and whose input position is inside the
//    image. The others load from the tensor's first pixel (an address
//    that always exists) and are zeroed when the unit is stored.
//  - the columns are strips of 64: a row of dW is taps * ceil(C/64)
//    strips, strip j being tap j % taps of channels 64*(j / taps).., and
//    every wave column of a block owns one strip with a tap and a first
//    channel of its own. A 64-channel 3x3 layer fills a 64x256 tile with
//    four taps, and the strips that re-read the same rows of x sit next
//    to each other. A strip beyond the last loads zeros, stores nothing.
// dW is written as [K][R][S][C], the memory of a channels-last (K,C,R,S)
// tensor; the workspace is [S][K][taps*C] and wrw_reduce_kernel is the
// same.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <c10/cuda/CUDAGuard.h>

#include <algorithm>
#include <vector>

#include "cast_common.h"

namespace {

constexpr int kThreads = 256;      // four waves
constexpr int kPT = 32;            // pixels per tile: two MFMA k-steps
constexpr int kRowBytes = 80;      // LDS row: 32 bf16 + 16 bytes padding
constexpr int kWave = 64;          // a wave's sub-tile is 64 x 64
constexpr int kTargetBlocks = 512; // grid size the S rule aims at
constexpr int kMinSlice = 256;     // pixels: a slice is never shorter

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

// ---------------------------------------------------------------- plan
struct WrwPlan {
  int TM, TN;      // tile rows (K) and columns (C)
  int tiles_m, tiles_n;
  long long L;     // pixels per slice, a multiple of kPT
  int S;           // slices
};

inline long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// The tile shape is the one of {128x128, 256x64, 64x256} that reads the
// fewest operand bytes, K * ceil(C/TN) + C * ceil(K/TM) per pixel (ties:
// in that order). The slice length is what brings the grid to about
// kTargetBlocks blocks, rounded up to whole pixel tiles and not below
// kMinSlice; S follows from it, so only the last slice can be short.
// With taps > 1 (wrw_gemm_conv) the columns are counted in strips of 64,
// taps * ceil(C/64) of them, and a pixel's x bytes in taps * C; with
// taps == 1 both are what they were.
WrwPlan wrw_plan(long long P, int C, int K, int taps = 1) {
  static const int shapes[3][2] = {{128, 128}, {256, 64}, {64, 256}};
  WrwPlan pl{};
  long long best = -1;
  const long long strips = taps * ceil_div(C, kWave);
  for (const auto& sh : shapes) {
    const long long tm = ceil_div(K, sh[0]);
    const long long tn = ceil_div(strips, sh[1] / kWave);
    const long long cost = (long long)K * tn + (long long)taps * C * tm;
    if (best < 0 || cost < best) {
      best = cost;
      pl.TM = sh[0];
      pl.TN = sh[1];
      pl.tiles_m = (int)tm;
      pl.tiles_n = (int)tn;
    }
  }
  const long long tiles = (long long)pl.tiles_m * pl.tiles_n;
  const long long want = ceil_div(kTargetBlocks, tiles);
  pl.L = std::max<long long>(kMinSlice,
                             ceil_div(ceil_div(P, want), kPT) * kPT);
  pl.S = (int)ceil_div(P, pl.L);
  return pl;
}

// ------------------------------------------------------------- loading
// One unit: 8 channels (one 16-byte group) of 8 consecutive pixels.
struct Unit {
  uint4 px[8];
  unsigned int mask;  // bit j: px[j] exists; the others are read as zero
};

// src is [P][nch]; a group beyond nch or a pixel beyond pend is zero.
// The pixels that do not exist re-read the last one that does (never
// past it) and are masked when the unit is stored: the eight loads are
// straight-line code and nothing here waits for them.
__device__ __forceinline__ void unit_load(Unit& u,
                                          const unsigned short* __restrict__ src,
                                          long long p0, long long pend,
                                          int ch, int nch) {
  const long long left = pend - p0;
  const int nv = ch < nch ? (int)(left < 0 ? 0 : left > 8 ? 8 : left) : 0;
  u.mask = (1u << nv) - 1u;
  if (nv == 0) {
#pragma unroll
    for (int j = 0; j < 8; j++) u.px[j] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  const unsigned short* at = src + p0 * (long long)nch + ch;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int jj = j < nv ? j : nv - 1;
    u.px[j] = *reinterpret_cast<const uint4*>(at + (long long)jj * nch);
  }
}

// The gathered operand of wrw_conv_kernel. Uniform over the grid:
struct ConvGeom {
  int H, W, Ho, Wo;  // input and output image
  int st;            // stride
  int R, taps;       // kernel side, R * R
  int pad;
  int nstrips;       // taps * ceil(C / 64)
  int dw, dh, dn;    // 32 output pixels on: wo += dw, ho += dh, n += dn,
                     // before the carries (32 = (dn*Ho + dh)*Wo + dw)
};

// A loading thread's place in the output image: pixel q is (n, ho, wo).
struct Walk {
  int n, ho, wo;
  unsigned int q;
};

__device__ __forceinline__ void walk_begin(Walk& w, const ConvGeom& g,
                                           unsigned int q) {
  const unsigned int row = q / (unsigned int)g.Wo;
  w.q = q;
  w.wo = (int)(q - row * (unsigned int)g.Wo);
  w.n = (int)(row / (unsigned int)g.Ho);
  w.ho = (int)(row - (unsigned int)w.n * (unsigned int)g.Ho);
}

// 32 pixels on. wo < 2*Wo and ho < 2*Ho before their carries, so one
// subtraction each is enough.
__device__ __forceinline__ void walk_tile(Walk& w, const ConvGeom& g) {
  w.q += kPT;
  w.wo += g.dw;
  const int cw = w.wo >= g.Wo;
  w.wo -= cw ? g.Wo : 0;
  w.ho += g.dh + cw;
  const int chh = w.ho >= g.Ho;
  w.ho -= chh ? g.Ho : 0;
  w.n += g.dn + chh;
}

// x is [N][H][W][C]; the unit is channels ch..ch+7 of tap (r, s) =
// (roff + pad, soff + pad) at the 8 output pixels from w on. Pixel j is
// valid when it is below qend and its input position is inside the image
// (its own image: hi and wi are tested, not the flat index, so a shifted
// pixel never lands in a neighbour). An invalid pixel loads x's first
// pixel instead. Pixel indices are 32-bit (N*H*W < 2^31), offsets 64-bit.
__device__ __forceinline__ void unit_gather(Unit& u,
                                            const unsigned short* __restrict__ x,
                                            const ConvGeom& g, const Walk& w,
                                            unsigned int qend, int roff,
                                            int soff, int ch, int C,
                                            bool group) {
  u.mask = 0u;
  if (!group) {
#pragma unroll
    for (int j = 0; j < 8; j++) u.px[j] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  const unsigned short* at = x + ch;
  int n = w.n, ho = w.ho, wo = w.wo;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int hi = ho * g.st + roff, wi = wo * g.st + soff;
    const bool ok = w.q + j < qend && (unsigned int)hi < (unsigned int)g.H &&
                    (unsigned int)wi < (unsigned int)g.W;
    const unsigned int pix =
        ((unsigned int)n * (unsigned int)g.H + (unsigned int)hi) *
            (unsigned int)g.W + (unsigned int)wi;
    u.mask |= (ok ? 1u : 0u) << j;
    u.px[j] = *reinterpret_cast<const uint4*>(
        at + (long long)(ok ? pix : 0u) * C);
    wo++;
    const bool cw = wo == g.Wo;
    wo = cw ? 0 : wo;
    ho += cw;
    const bool chh = ho == g.Ho;
    ho = chh ? 0 : ho;
    n += chh;
  }
}

__device__ __forceinline__ unsigned int word_of(const uint4& v, int d) {
  return d == 0 ? v.x : d == 1 ? v.y : d == 2 ? v.z : v.w;
}

// Transposes the unit in registers and writes channel c's 8 pixels as one
// 16-byte row segment: row[c] points at channel c's pixel octet.
__device__ __forceinline__ void unit_store(const Unit& u, char* row0) {
#pragma unroll
  for (int c = 0; c < 8; c++) {
    const int d = c >> 1;
    unsigned int w[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const unsigned int lo =
          (u.mask >> (2 * i)) & 1u ? word_of(u.px[2 * i], d) : 0u;
      const unsigned int hi =
          (u.mask >> (2 * i + 1)) & 1u ? word_of(u.px[2 * i + 1], d) : 0u;
      w[i] = (c & 1) ? ((lo >> 16) | (hi & 0xffff0000u))
                     : ((lo & 0xffffu) | (hi << 16));
    }
    *reinterpret_cast<uint4*>(row0 + c * kRowBytes) =
        make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// ------------------------------------------------------------ the GEMM
// WM x WN waves, WM * WN == 4; the block's tile is (64*WM) x (64*WN).
// CONV: the B operand is gathered through cg and the columns are strips
// (wrw_conv_kernel); P is then the number of output pixels and tiles_n
// counts tiles of WN strips. Without CONV cg is not read.
template <int WM, int WN, bool CONV>
__device__ __forceinline__ void wrw_gemm_body(
    const unsigned short* __restrict__ x,
    const unsigned short* __restrict__ dy, float* __restrict__ ws,
    unsigned short* __restrict__ out, long long P, int C, int K, long long L,
    int tiles_n, const ConvGeom& cg) {
  constexpr int TM = kWave * WM, TN = kWave * WN;
  constexpr int ROWS = TM + TN;            // A rows, then B rows
  constexpr int GA = TM / 8, GB = TN / 8;  // channel groups per operand
  constexpr int UNITS = (GA + GB) * (kPT / 8);
  static_assert(WM * WN == 4 && UNITS <= kThreads, "one unit per thread");
  __shared__ __attribute__((aligned(16))) char lds[2][ROWS * kRowBytes];

  const int tid = threadIdx.x;
  const int tile = blockIdx.x;
  const int m0 = (tile / tiles_n) * TM;  // first dW row (K)
  const int n0 = (tile % tiles_n) * TN;  // first dW column (C)
  const long long s = blockIdx.y;
  const long long pbeg = s * L;
  const long long pend = pbeg + L < P ? pbeg + L : P;
  const int T = (int)((pend - pbeg + kPT - 1) / kPT);

  // this thread's unit: operand, channel group, pixel octet; lanes next
  // to each other take neighbouring groups of one pixel
  const bool loader = tid < UNITS;
  const bool is_a = tid < GA * (kPT / 8);
  const int ub = is_a ? tid : tid - GA * (kPT / 8);
  const int ng = is_a ? GA : GB;
  const int g = ub % ng, oct = ub / ng;
  const unsigned short* src = is_a ? dy : x;
  const int nch = is_a ? K : C;
  int ch = (is_a ? m0 : n0) + 8 * g;
  const int row = (is_a ? 0 : TM) + 8 * g;
  const int unit_off = row * kRowBytes + oct * 16;
  // CONV: a B unit belongs to the strip of its wave column (8 groups a
  // strip): tap strip % taps of the channels from 64 * (strip / taps)
  Walk walk{};
  int roff = 0, soff = 0;
  bool group = false;
  if constexpr (CONV) {
    if (!is_a) {
      const int strip = (tile % tiles_n) * WN + g / 8;
      const int tap = strip % cg.taps;
      ch = (strip / cg.taps) * kWave + 8 * (g % 8);
      group = loader && strip < cg.nstrips && ch < C;
      roff = tap / cg.R - cg.pad;
      soff = tap % cg.R - cg.pad;
      walk_begin(walk, cg, (unsigned int)pbeg + 8u * oct);
    }
  }
  // one unit of pixel tile t: A (and B without CONV) over consecutive
  // pixels, B with CONV gathered at walk
  auto load = [&](Unit& u, int t) {
    if (CONV && !is_a)
      unit_gather(u, x, cg, walk, (unsigned int)pend, roff, soff, ch, C,
                  group);
    else
      unit_load(u, src, pbeg + (long long)t * kPT + 8 * oct, pend, ch, nch);
  };

  // this lane's operand rows: A rows am + 32*i, B rows bn + 32*j
  const int wave = tid / 64, lane = tid % 64;
  const int am = (wave / WN) * kWave, bn = (wave % WN) * kWave;
  const int frag_off = (lane % 32) * kRowBytes + (lane / 32) * 16;
  const int a_off = am * kRowBytes + frag_off;
  const int b_off = (TM + bn) * kRowBytes + frag_off;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int v = 0; v < 16; v++) acc[i][j][v] = 0.0f;

  Unit u;
  if (loader) {
    load(u, 0);
    unit_store(u, lds[0] + unit_off);
  }
  __syncthreads();

  for (int t = 0; t < T; t++) {
    const bool more = t + 1 < T;
    if constexpr (CONV) walk_tile(walk, cg);
    if (more && loader) load(u, t + 1);
    const char* cur = lds[t & 1];
#pragma unroll
    for (int kk = 0; kk < kPT / 16; kk++) {
      bf16x8 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; i++) {
        a[i] = *reinterpret_cast<const bf16x8*>(
            cur + a_off + i * 32 * kRowBytes + kk * 32);
        b[i] = *reinterpret_cast<const bf16x8*>(
            cur + b_off + i * 32 * kRowBytes + kk * 32);
      }
#pragma unroll
      for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (more && loader) unit_store(u, lds[(t + 1) & 1] + unit_off);
    __syncthreads();
  }

  // accumulator register v of lane l: row 8*(v/4) + 4*(l/32) + v%4,
  // column l%32 of its 32x32 tile
  const bool direct = ws == nullptr;  // S == 1: round here
  // a dW row: C columns, or with CONV [taps][C], this wave's strip at
  // tap * C + its first channel (cbase); cend ends the strip's channels
  int ld = C, cbase = n0 + bn, cend = C;
  if constexpr (CONV) {
    const int strip = (tile % tiles_n) * WN + wave % WN;
    const int c0 = (strip / cg.taps) * kWave;
    ld = cg.taps * C;
    cbase = (strip % cg.taps) * C + c0;
    cend = strip < cg.nstrips ? cbase + (C - c0) : 0;
  }
  float* wsl = direct ? nullptr : ws + s * (long long)K * ld;
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int c = cbase + 32 * j + lane % 32;
#pragma unroll
      for (int v = 0; v < 16; v++) {
        const int k = m0 + am + 32 * i + 8 * (v / 4) + 4 * (lane / 32) + v % 4;
        if (k < K && c < cend) {
          const long long at = (long long)k * ld + c;
          if (direct)
            out[at] = cast_f32_to_bf16(acc[i][j][v]);
          else
            wsl[at] = acc[i][j][v];
        }
      }
    }
}

template <int WM, int WN>
__global__ void __launch_bounds__(kThreads)
wrw_gemm_kernel(const unsigned short* __restrict__ x,
                const unsigned short* __restrict__ dy,
                float* __restrict__ ws, unsigned short* __restrict__ out,
                long long P, int C, int K, long long L, int tiles_n) {
  wrw_gemm_body<WM, WN, false>(x, dy, ws, out, P, C, K, L, tiles_n,
                               ConvGeom{});
}

// Q output pixels; x is [N][H][W][C], dy [Q][K], dW and the workspace
// slices [K][taps][C].
template <int WM, int WN>
__global__ void __launch_bounds__(kThreads)
wrw_conv_kernel(const unsigned short* __restrict__ x,
                const unsigned short* __restrict__ dy,
                float* __restrict__ ws, unsigned short* __restrict__ out,
                long long Q, int C, int K, long long L, int tiles_n,
                ConvGeom cg) {
  wrw_gemm_body<WM, WN, true>(x, dy, ws, out, Q, C, K, L, tiles_n, cg);
}

// dW[e] = bf16(sum over s of ws[s][e]) in a fixed order: the slices are
// cut into kChunks runs of ceil(S / kChunks) consecutive slices, a run is
// added in slice order and the runs are added in order. A block takes 16
// pairs of elements (K*C is a multiple of 64) and gives each run to one
// 16-lane row of its threads: with one output tile S is in the hundreds
// and the output small, and one thread per pair walking all of S left the
// machine waiting on a few long chains of loads.
constexpr int kChunks = 16, kPairs = kThreads / kChunks;

__global__ void __launch_bounds__(kThreads)
wrw_reduce_kernel(const float* __restrict__ ws,
                  unsigned int* __restrict__ out, long long pairs, int S) {
  __shared__ float2 part[kChunks][kPairs];
  const int lane = threadIdx.x % kPairs, chunk = threadIdx.x / kPairs;
  const long long e = (long long)blockIdx.x * kPairs + lane;  // < pairs
  const int per = (S + kChunks - 1) / kChunks;
  const int s0 = chunk * per, s1 = s0 + per < S ? s0 + per : S;
  const float2* at = reinterpret_cast<const float2*>(ws) + e;
  float2 sum = make_float2(0.0f, 0.0f);
  if (s0 < S) sum = at[(long long)s0 * pairs];
#pragma unroll 8
  for (int s = s0 + 1; s < s1; s++) {
    const float2 v = at[(long long)s * pairs];
    sum.x += v.x;
    sum.y += v.y;
  }
  part[chunk][lane] = sum;
  __syncthreads();
  if (chunk != 0) return;
  const int runs = (S + per - 1) / per;
  for (int c = 1; c < runs; c++) {
    sum.x += part[c][lane].x;
    sum.y += part[c][lane].y;
  }
  out[e] = (unsigned int)cast_f32_to_bf16(sum.x) |
           ((unsigned int)cast_f32_to_bf16(sum.y) << 16);
}

template <int WM, int WN>
void launch_gemm(const WrwPlan& pl, hipStream_t stream,
                 const unsigned short* x, const unsigned short* dy, float* ws,
                 unsigned short* out, long long P, int C, int K) {
  hipLaunchKernelGGL((wrw_gemm_kernel<WM, WN>),
                     dim3((uint32_t)(pl.tiles_m * pl.tiles_n),
                          (uint32_t)pl.S),
                     dim3(kThreads), 0, stream, x, dy, ws, out, P, C, K, pl.L,
                     pl.tiles_n);
}

template <int WM, int WN>
void launch_conv(const WrwPlan& pl, hipStream_t stream,
                 const unsigned short* x, const unsigned short* dy, float* ws,
                 unsigned short* out, long long Q, int C, int K,
                 const ConvGeom& cg) {
  hipLaunchKernelGGL((wrw_conv_kernel<WM, WN>),
                     dim3((uint32_t)(pl.tiles_m * pl.tiles_n),
                          (uint32_t)pl.S),
                     dim3(kThreads), 0, stream, x, dy, ws, out, Q, C, K, pl.L,
                     pl.tiles_n, cg);
}

// dW = bf16(sum of the S workspace slices), `elems` elements each
void launch_reduce(hipStream_t stream, const float* ws, unsigned short* out,
                   long long elems, int S) {
  const long long pairs = elems / 2;
  hipLaunchKernelGGL(wrw_reduce_kernel, dim3((uint32_t)(pairs / kPairs)),
                     dim3(kThreads), 0, stream, ws,
                     reinterpret_cast<unsigned int*>(out), pairs, S);
}

bool channels_ok(int64_t n) { return n % 8 == 0 && n >= 8 && n <= 2048; }

// what both entry points ask of x and dy before they look at shapes
void check_operands(const char* name, const torch::Tensor& x,
                    const torch::Tensor& dy) {
  TORCH_CHECK(x.is_cuda() && dy.is_cuda() && x.dim() == 4 && dy.dim() == 4 &&
                  x.get_device() == dy.get_device(),
              name, ": 4-d tensors on one GPU expected");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 &&
                  dy.scalar_type() == at::kBFloat16,
              name, ": bf16 x and dy expected");
}

}  // namespace

// What wrw_gemm_1x1 accepts of a channel count (conv_split.hip asks).
bool wrw_gemm_channels_ok(int64_t c, int64_t k) {
  return channels_ok(c) && channels_ok(k);
}

// The (kernel, stride, padding) wrw_gemm_conv covers.
bool wrw_gemm_conv_geometry_ok(int64_t k, int64_t st, int64_t p) {
  return (k == 1 && p == 0 && (st == 1 || st == 2)) ||
         (k == 3 && p == 1 && (st == 1 || st == 2));
}

// {TM, TN, S, L} for P pixels (output pixels with taps > 1), C input and
// K output channels and a kernel of `taps` taps.
std::vector<int64_t> wrw_gemm_plan(int64_t P, int64_t C, int64_t K,
                                   int64_t taps) {
  TORCH_CHECK(P >= 1 && wrw_gemm_channels_ok(C, K) &&
                  (taps == 1 || taps == 9),
              "wrw_gemm_plan: P >= 1, channel counts that are multiples "
              "of 8 in [8, 2048] and 1 or 9 taps expected");
  const WrwPlan pl = wrw_plan(P, (int)C, (int)K, (int)taps);
  return {pl.TM, pl.TN, pl.S, pl.L};
}

// dW (K, C, 1, 1) of a stride-1 1x1 convolution from x (N, C, H, W) and
// dy (N, K, H, W), both dense channels-last bf16 on one device. Launches
// on the current stream, allocates through the caching allocator, no host
// sync.
torch::Tensor wrw_gemm_1x1(torch::Tensor x, torch::Tensor dy) {
  const char* name = "wrw_gemm_1x1";
  check_operands(name, x, dy);
  TORCH_CHECK(x.size(0) == dy.size(0) && x.size(2) == dy.size(2) &&
                  x.size(3) == dy.size(3),
              name, ": x and dy differ in N, H or W");
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast) &&
                  dy.is_contiguous(at::MemoryFormat::ChannelsLast),
              name, ": dense channels-last x and dy expected");
  const int64_t C = x.size(1), K = dy.size(1);
  const int64_t P = x.size(0) * x.size(2) * x.size(3);
  TORCH_CHECK(wrw_gemm_channels_ok(C, K) && P >= 1, name,
              ": unsupported shape: C and K must be multiples of 8 in "
              "[8, 2048] and P >= 1");
  c10::cuda::CUDAGuard device_guard(x.device());
  auto stream = at::cuda::getCurrentCUDAStream();
  // the strides at::convolution_backward reports for this weight
  // gradient: channels-last where the strides of x or dy say so, else
  // (H = W = 1 leaves that open) contiguous; the same memory either way
  const bool nhwc =
      x.suggest_memory_format() == at::MemoryFormat::ChannelsLast ||
      dy.suggest_memory_format() == at::MemoryFormat::ChannelsLast;
  torch::Tensor out = at::empty({K, C, 1, 1}, x.options(),
                                nhwc ? at::MemoryFormat::ChannelsLast
                                     : at::MemoryFormat::Contiguous);
  const WrwPlan pl = wrw_plan(P, (int)C, (int)K);
  torch::Tensor ws;
  float* wsp = nullptr;
  if (pl.S > 1) {
    ws = at::empty({pl.S, K, C}, x.options().dtype(at::kFloat));
    wsp = ws.data_ptr<float>();
  }
  const auto* xp = static_cast<const unsigned short*>(x.data_ptr());
  const auto* dyp = static_cast<const unsigned short*>(dy.data_ptr());
  auto* op = static_cast<unsigned short*>(out.data_ptr());
  TORCH_CHECK(((uintptr_t)xp | (uintptr_t)dyp) % 16 == 0, name,
              ": x and dy must start on a 16-byte boundary");
  if (pl.TM == 128)
    launch_gemm<2, 2>(pl, stream.stream(), xp, dyp, wsp, op, P, (int)C,
                      (int)K);
  else if (pl.TM == 256)
    launch_gemm<4, 1>(pl, stream.stream(), xp, dyp, wsp, op, P, (int)C,
                      (int)K);
  else
    launch_gemm<1, 4>(pl, stream.stream(), xp, dyp, wsp, op, P, (int)C,
                      (int)K);
  if (pl.S > 1) launch_reduce(stream.stream(), wsp, op, K * C, pl.S);
  return out;
}

// dW (K, C, k, k), dense channels-last ([K][k][k][C]), of a convolution
// with a square k x k kernel, stride `stride` and zero padding `padding`
// (wrw_gemm_conv_geometry_ok), dilation 1, groups 1, from dense
// channels-last bf16 x (N, C, H, W) and dy (N, K, Ho, Wo). (1, 1, 0) is
// wrw_gemm_1x1. Same stream, allocator and no-sync rules.
torch::Tensor wrw_gemm_conv(torch::Tensor x, torch::Tensor dy,
                            int64_t kernel, int64_t stride, int64_t padding) {
  const char* name = "wrw_gemm_conv";
  TORCH_CHECK(wrw_gemm_conv_geometry_ok(kernel, stride, padding), name,
              ": (kernel, stride, padding) must be one of (1,1,0), (3,1,1), "
              "(1,2,0), (3,2,1)");
  if (kernel == 1 && stride == 1) return wrw_gemm_1x1(x, dy);
  check_operands(name, x, dy);
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int64_t K = dy.size(1);
  const int64_t Ho = (H + 2 * padding - kernel) / stride + 1;
  const int64_t Wo = (W + 2 * padding - kernel) / stride + 1;
  TORCH_CHECK(N >= 1 && H >= 1 && W >= 1 && N * H * W < (1LL << 31), name,
              ": x needs at least one pixel and N*H*W below 2^31");
  TORCH_CHECK(Ho >= 1 && Wo >= 1 && dy.size(0) == N && dy.size(2) == Ho &&
                  dy.size(3) == Wo,
              name, ": dy is not (N, K, Ho, Wo) of this convolution of x");
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast) &&
                  dy.is_contiguous(at::MemoryFormat::ChannelsLast),
              name, ": dense channels-last x and dy expected");
  TORCH_CHECK(wrw_gemm_channels_ok(C, K), name,
              ": unsupported shape: C and K must be multiples of 8 in "
              "[8, 2048]");
  c10::cuda::CUDAGuard device_guard(x.device());
  auto stream = at::cuda::getCurrentCUDAStream();
  const int64_t taps = kernel * kernel;
  // a 1x1 weight's strides: as wrw_gemm_1x1 chooses them
  const bool nhwc =
      kernel > 1 ||
      x.suggest_memory_format() == at::MemoryFormat::ChannelsLast ||
      dy.suggest_memory_format() == at::MemoryFormat::ChannelsLast;
  torch::Tensor out = at::empty({K, C, kernel, kernel}, x.options(),
                                nhwc ? at::MemoryFormat::ChannelsLast
                                     : at::MemoryFormat::Contiguous);
  const long long Q = N * Ho * Wo;
  const WrwPlan pl = wrw_plan(Q, (int)C, (int)K, (int)taps);
  ConvGeom cg{};
  cg.H = (int)H, cg.W = (int)W, cg.Ho = (int)Ho, cg.Wo = (int)Wo;
  cg.st = (int)stride, cg.R = (int)kernel, cg.taps = (int)taps;
  cg.pad = (int)padding;
  cg.nstrips = (int)(taps * ceil_div(C, kWave));
  cg.dw = kPT % cg.Wo;
  cg.dh = (kPT / cg.Wo) % cg.Ho;
  cg.dn = (kPT / cg.Wo) / cg.Ho;
  torch::Tensor ws;
  float* wsp = nullptr;
  if (pl.S > 1) {
    ws = at::empty({pl.S, K, taps * C}, x.options().dtype(at::kFloat));
    wsp = ws.data_ptr<float>();
  }
  const auto* xp = static_cast<const unsigned short*>(x.data_ptr());
  const auto* dyp = static_cast<const unsigned short*>(dy.data_ptr());
  auto* op = static_cast<unsigned short*>(out.data_ptr());
  TORCH_CHECK(((uintptr_t)xp | (uintptr_t)dyp) % 16 == 0, name,
              ": x and dy must start on a 16-byte boundary");
  if (pl.TM == 128)
    launch_conv<2, 2>(pl, stream.stream(), xp, dyp, wsp, op, Q, (int)C,
                      (int)K, cg);
  else if (pl.TM == 256)
    launch_conv<4, 1>(pl, stream.stream(), xp, dyp, wsp, op, Q, (int)C,
                      (int)K, cg);
  else
    launch_conv<1, 4>(pl, stream.stream(), xp, dyp, wsp, op, Q, (int)C,
                      (int)K, cg);
  if (pl.S > 1) launch_reduce(stream.stream(), wsp, op, K * taps * C, pl.S);
  return out;
}
