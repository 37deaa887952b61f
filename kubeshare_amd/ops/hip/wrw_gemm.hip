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
WrwPlan wrw_plan(long long P, int C, int K) {
  static const int shapes[3][2] = {{128, 128}, {256, 64}, {64, 256}};
  WrwPlan pl{};
  long long best = -1;
  for (const auto& sh : shapes) {
    const long long tm = ceil_div(K, sh[0]), tn = ceil_div(C, sh[1]);
    const long long cost = (long long)K * tn + (long long)C * tm;
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
  int nv;  // pixels that exist; px[nv..] are to be read as zero
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
  u.nv = ch < nch ? (int)(left < 0 ? 0 : left > 8 ? 8 : left) : 0;
  if (u.nv == 0) {
#pragma unroll
    for (int j = 0; j < 8; j++) u.px[j] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  const unsigned short* at = src + p0 * (long long)nch + ch;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int jj = j < u.nv ? j : u.nv - 1;
    u.px[j] = *reinterpret_cast<const uint4*>(at + (long long)jj * nch);
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
      const unsigned int lo = 2 * i < u.nv ? word_of(u.px[2 * i], d) : 0u;
      const unsigned int hi =
          2 * i + 1 < u.nv ? word_of(u.px[2 * i + 1], d) : 0u;
      w[i] = (c & 1) ? ((lo >> 16) | (hi & 0xffff0000u))
                     : ((lo & 0xffffu) | (hi << 16));
    }
    *reinterpret_cast<uint4*>(row0 + c * kRowBytes) =
        make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// ------------------------------------------------------------ the GEMM
// WM x WN waves, WM * WN == 4; the block's tile is (64*WM) x (64*WN).
template <int WM, int WN>
__global__ void __launch_bounds__(kThreads)
wrw_gemm_kernel(const unsigned short* __restrict__ x,
                const unsigned short* __restrict__ dy,
                float* __restrict__ ws, unsigned short* __restrict__ out,
                long long P, int C, int K, long long L, int tiles_n) {
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
  const int ch = (is_a ? m0 : n0) + 8 * g;
  const int row = (is_a ? 0 : TM) + 8 * g;
  const int unit_off = row * kRowBytes + oct * 16;

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
    unit_load(u, src, pbeg + 8 * oct, pend, ch, nch);
    unit_store(u, lds[0] + unit_off);
  }
  __syncthreads();

  for (int t = 0; t < T; t++) {
    const bool more = t + 1 < T;
    if (more && loader)
      unit_load(u, src, pbeg + (long long)(t + 1) * kPT + 8 * oct, pend, ch,
                nch);
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
  float* wsl = direct ? nullptr : ws + s * (long long)K * C;
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int c = n0 + bn + 32 * j + lane % 32;
#pragma unroll
      for (int v = 0; v < 16; v++) {
        const int k = m0 + am + 32 * i + 8 * (v / 4) + 4 * (lane / 32) + v % 4;
        if (k < K && c < C) {
          const long long at = (long long)k * C + c;
          if (direct)
            out[at] = cast_f32_to_bf16(acc[i][j][v]);
          else
            wsl[at] = acc[i][j][v];
        }
      }
    }
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

bool channels_ok(int64_t n) { return n % 8 == 0 && n >= 8 && n <= 2048; }

}  // namespace

// What wrw_gemm_1x1 accepts of a channel count (conv_split.hip asks).
bool wrw_gemm_channels_ok(int64_t c, int64_t k) {
  return channels_ok(c) && channels_ok(k);
}

// {TM, TN, S, L} for P pixels, C input and K output channels.
std::vector<int64_t> wrw_gemm_plan(int64_t P, int64_t C, int64_t K) {
  TORCH_CHECK(P >= 1 && wrw_gemm_channels_ok(C, K),
              "wrw_gemm_plan: P >= 1 and channel counts that are multiples "
              "of 8 in [8, 2048] expected");
  const WrwPlan pl = wrw_plan(P, (int)C, (int)K);
  return {pl.TM, pl.TN, pl.S, pl.L};
}

// dW (K, C, 1, 1) of a stride-1 1x1 convolution from x (N, C, H, W) and
// dy (N, K, H, W), both dense channels-last bf16 on one device. Launches
// on the current stream, allocates through the caching allocator, no host
// sync.
torch::Tensor wrw_gemm_1x1(torch::Tensor x, torch::Tensor dy) {
  const char* name = "wrw_gemm_1x1";
  TORCH_CHECK(x.is_cuda() && dy.is_cuda() && x.dim() == 4 && dy.dim() == 4 &&
                  x.get_device() == dy.get_device(),
              name, ": 4-d tensors on one GPU expected");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 &&
                  dy.scalar_type() == at::kBFloat16,
              name, ": bf16 x and dy expected");
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
  if (pl.S > 1) {
    const long long pairs = K * C / 2;
    hipLaunchKernelGGL(wrw_reduce_kernel, dim3((uint32_t)(pairs / kPairs)),
                       dim3(kThreads), 0, stream.stream(), wsp,
                       reinterpret_cast<unsigned int*>(op), pairs, pl.S);
  }
  return out;
}
