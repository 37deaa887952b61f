// kubeshare_amd fused HIP ops for gfx950 (CDNA4, wave64).
//
// Built in-tree via torch.utils.cpp_extension (PYTORCH_ROCM_ARCH=gfx950);
// kubeshare_amd.ops refuses to import without this extension on a GPU
// box (fail-loud policy).
//
// Kernels:
//  - burn_kernel: wall-clock-bounded MFMA/VALU spin — a *calibrated GPU
//    load generator* for the isolation tests and rocprof quota proofs
//    (occupies all CUs for a requested number of microseconds).
//  - sgd_mom_f32_kernel: SGD+momentum on one f32 tensor, grid-stride,
//    float4-vectorized (guide G13: vectorize ANY memory-bound op). Kept
//    as the bit-exact reference and for KUBESHARE_SGD_MULTI=0.
//  - sgd_mom_multi_f32_kernel: the same update for up to 110 tensors per
//    launch; pointers and block prefix sums ride in the kernel arguments
//    (ResNet50's 161 tensors: 2 launches instead of 161). Templated on
//    the gradient type: f32, or bf16 from a bf16 gradient bucket.
//  - grad_bucket.hip: multi-tensor pack / unpack between per-parameter
//    gradients and the flat bucket a gang all-reduces (bound below).
//  - bn_relu.hip / pool.hip / cast.hip: fused NHWC bf16 BN+ReLU(+add),
//    max-pool and the multi-tensor f32 <-> bf16 casts (bound below).
//  - bn_pool.hip: BN+ReLU+max-pool in one op, the full-resolution
//    activation never written (ResNet stem, VGG pools).
//  - bn_join.hip: a downsample block's two BNs, the residual add and the
//    ReLU in one op; the downsample BN's output is never written.
//  - bias_relu.hip: bias+ReLU(+max-pool) for conv layers without a BN
//    (the plain VGG16), bias gradient in the same backward pass.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <type_traits>
#include <vector>

#define WAVE 64

// ---------------------------------------------------------------- burn
// Spin for ~`ticks` of the 100 MHz constant wallclock. Each workgroup
// spins independently; 64 f32 FMAs per poll keep the VALU pipes busy so
// SQ_BUSY/GRBM counters register genuine occupancy.
__global__ void burn_kernel(long long ticks, float* sink) {
  long long start = wall_clock64();
  float acc = threadIdx.x * 1e-9f;
  while (wall_clock64() - start < ticks) {
#pragma unroll
    for (int i = 0; i < 64; i++) acc = fmaf(acc, 1.0000001f, 1e-12f);
  }
  if (acc == 12345.678f) sink[0] = acc;  // never true: keeps acc alive
}

// Occupy the whole chip (256 CUs, a few blocks each) for ~ms
// milliseconds on the current stream.
void burn(double ms, int64_t blocks, int64_t threads) {
  // gfx950 wall_clock64 runs at 100 MHz
  long long ticks = (long long)(ms * 100000.0);
  auto stream = at::cuda::getCurrentCUDAStream();
  static float* sink = nullptr;
  if (!sink) {
    if (hipMalloc(&sink, sizeof(float)) != hipSuccess)
      throw std::runtime_error("burn: hipMalloc failed");
  }
  hipLaunchKernelGGL(burn_kernel, dim3((uint32_t)blocks),
                     dim3((uint32_t)threads), 0, stream.stream(), ticks,
                     sink);
}

// ------------------------------------------------- fused SGD + momentum
// v = mu*v + g + wd*p ; p -= lr*v       (PyTorch SGD semantics,
// momentum buffer already initialized; dampening=0, nesterov=false)
template <typename T>
struct Vec4;
template <>
struct Vec4<float> {
  using type = float4;
};

// The one place the update is spelled out, shared by the per-tensor and
// the multi-tensor kernel. The FMAs are explicit: left to -ffp-contract
// the backend fused `mu*v + g + wd*p` in the float4 loops but emitted a
// packed multiply and two adds in the scalar loops, so an element's
// last bit depended on which loop it fell into. This is the float4
// loops' sequence, now used for every element.
__device__ __forceinline__ void sgd_mom_update(float& p, float g, float& v,
                                               float lr, float mu, float wd) {
  v = fmaf(wd, p, fmaf(mu, v, g));
  p = fmaf(-lr, v, p);
}

__device__ __forceinline__ void sgd_mom_update4(float4& p, const float4& g,
                                                float4& v, float lr, float mu,
                                                float wd) {
  sgd_mom_update(p.x, g.x, v.x, lr, mu, wd);
  sgd_mom_update(p.y, g.y, v.y, lr, mu, wd);
  sgd_mom_update(p.z, g.z, v.z, lr, mu, wd);
  sgd_mom_update(p.w, g.w, v.w, lr, mu, wd);
}

__global__ void sgd_mom_f32_kernel(float* __restrict__ p,
                                   const float* __restrict__ g,
                                   float* __restrict__ v, float lr, float mu,
                                   float wd, long long n) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  long long n4 = n / 4;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  float4* p4 = reinterpret_cast<float4*>(p);
  float4* v4 = reinterpret_cast<float4*>(v);
  for (long long k = i; k < n4; k += stride) {
    float4 pv = p4[k], gv = g4[k], vv = v4[k];
    sgd_mom_update4(pv, gv, vv, lr, mu, wd);
    v4[k] = vv;
    p4[k] = pv;
  }
  // tail
  for (long long k = n4 * 4 + i; k < n; k += stride) {
    float pv = p[k], vv = v[k];
    sgd_mom_update(pv, g[k], vv, lr, mu, wd);
    v[k] = vv;
    p[k] = pv;
  }
}

// ------------------------------------------------ multi-tensor variant
// One launch updates up to KS_SGD_MAX_TENSORS (p, g, v) triples. The
// pointers, element counts and a prefix sum of per-tensor block counts
// travel BY VALUE in the kernel arguments (4096-byte limit): there is no
// device-side pointer table that could go stale between steps. A block
// binary-searches the prefix sum for its tensor and owns one
// KS_SGD_CHUNK-element chunk of it.
#define KS_SGD_THREADS 256
#define KS_SGD_VPT 4  // float4 per thread: 4 independent 16-B loads x 3
#define KS_SGD_CHUNK (KS_SGD_THREADS * KS_SGD_VPT * 4)
#define KS_SGD_MAX_TENSORS 110

// G is the gradient's element type: float, or unsigned short holding
// bf16 bits (a bf16 ops.GradBucket's views), upcast in registers.
template <typename G>
struct SgdMultiArgs {
  float* p[KS_SGD_MAX_TENSORS];
  const G* g[KS_SGD_MAX_TENSORS];
  float* v[KS_SGD_MAX_TENSORS];
  long long n[KS_SGD_MAX_TENSORS];
  // blk[t] = first block of tensor t; blk[count] = grid size
  int blk[KS_SGD_MAX_TENSORS + 1];
  int count;
  float lr, mu, wd;
};
static_assert(sizeof(SgdMultiArgs<float>) <= 4096 &&
                  sizeof(SgdMultiArgs<unsigned short>) <= 4096,
              "SgdMultiArgs must fit the 4 KiB kernel-argument segment");

// four / one gradient element(s) as f32 (bf16 -> f32 is exact)
__device__ __forceinline__ float4 sgd_load_g4(const float* g, int k) {
  return reinterpret_cast<const float4*>(g)[k];
}
__device__ __forceinline__ float4 sgd_load_g4(const unsigned short* g,
                                              int k) {
  const ushort4 u = reinterpret_cast<const ushort4*>(g)[k];
  return make_float4(__uint_as_float((unsigned int)u.x << 16),
                     __uint_as_float((unsigned int)u.y << 16),
                     __uint_as_float((unsigned int)u.z << 16),
                     __uint_as_float((unsigned int)u.w << 16));
}
__device__ __forceinline__ float sgd_load_g(const float* g, int k) {
  return g[k];
}
__device__ __forceinline__ float sgd_load_g(const unsigned short* g, int k) {
  return __uint_as_float((unsigned int)g[k] << 16);
}

template <typename G>
__global__ void __launch_bounds__(KS_SGD_THREADS)
sgd_mom_multi_f32_kernel(const SgdMultiArgs<G> a) {
  const int b = blockIdx.x;
  // largest t with blk[t] <= b (blk is non-decreasing, blk[0] == 0,
  // b < blk[count]; tensors own >= 1 block, so the answer is unique)
  int lo = 0, hi = a.count - 1;
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (a.blk[mid] <= b) lo = mid; else hi = mid - 1;
  }
  float* __restrict__ p = a.p[lo];
  const G* __restrict__ g = a.g[lo];
  float* __restrict__ v = a.v[lo];
  const long long n = a.n[lo];
  const float lr = a.lr, mu = a.mu, wd = a.wd;
  const long long base = (long long)(b - a.blk[lo]) * KS_SGD_CHUNK;
  long long rem = n - base;  // > 0 by construction of blk
  const int len = rem < KS_SGD_CHUNK ? (int)rem : KS_SGD_CHUNK;
  p += base;
  g += base;
  v += base;
  const int tid = threadIdx.x;
  // base is a multiple of 4 elements, so the chunk start is 16-byte
  // aligned exactly when the tensor start is; misaligned views
  // (narrow() at an odd offset) take the scalar path. (Four gradient
  // elements are 16 bytes of f32, 8 of bf16.)
  const uintptr_t ga = (uintptr_t)g * (sizeof(float) / sizeof(G));
  const bool vec = (((uintptr_t)p | ga | (uintptr_t)v) & 15) == 0;
  if (vec) {
    const int len4 = len >> 2;
    float4* p4 = reinterpret_cast<float4*>(p);
    float4* v4 = reinterpret_cast<float4*>(v);
    if (len == KS_SGD_CHUNK) {
      float4 pv[KS_SGD_VPT], gv[KS_SGD_VPT], vv[KS_SGD_VPT];
#pragma unroll
      for (int u = 0; u < KS_SGD_VPT; u++) {
        const int k = tid + u * KS_SGD_THREADS;
        pv[u] = p4[k];
        gv[u] = sgd_load_g4(g, k);
        vv[u] = v4[k];
      }
#pragma unroll
      for (int u = 0; u < KS_SGD_VPT; u++) {
        const int k = tid + u * KS_SGD_THREADS;
        sgd_mom_update4(pv[u], gv[u], vv[u], lr, mu, wd);
        v4[k] = vv[u];
        p4[k] = pv[u];
      }
      return;
    }
    for (int k = tid; k < len4; k += KS_SGD_THREADS) {
      float4 pv = p4[k], gv = sgd_load_g4(g, k), vv = v4[k];
      sgd_mom_update4(pv, gv, vv, lr, mu, wd);
      v4[k] = vv;
      p4[k] = pv;
    }
    for (int k = len4 * 4 + tid; k < len; k += KS_SGD_THREADS) {
      float pv = p[k], vv = v[k];
      sgd_mom_update(pv, sgd_load_g(g, k), vv, lr, mu, wd);
      v[k] = vv;
      p[k] = pv;
    }
    return;
  }
  for (int k = tid; k < len; k += KS_SGD_THREADS) {
    float pv = p[k], vv = v[k];
    sgd_mom_update(pv, sgd_load_g(g, k), vv, lr, mu, wd);
    v[k] = vv;
    p[k] = pv;
  }
}

void sgd_momentum_(std::vector<torch::Tensor> params,
                   std::vector<torch::Tensor> grads,
                   std::vector<torch::Tensor> momenta, double lr, double mu,
                   double wd) {
  auto stream = at::cuda::getCurrentCUDAStream();
  for (size_t t = 0; t < params.size(); t++) {
    auto& p = params[t];
    auto& g = grads[t];
    auto& v = momenta[t];
    TORCH_CHECK(p.is_cuda() && p.scalar_type() == at::kFloat &&
                    p.is_non_overlapping_and_dense() &&
                    g.sizes() == p.sizes() && g.strides() == p.strides() &&
                    v.strides() == p.strides() &&
                    g.scalar_type() == at::kFloat &&
                    v.scalar_type() == at::kFloat,
                "sgd_momentum_: f32 dense tensors with matching strides "
                "(any memory format: the update is elementwise over the "
                "flat storage)");
    long long n = p.numel();
    int threads = 256;
    int blocks = (int)std::min<long long>(2048, (n / 4 + threads - 1) / threads + 1);
    hipLaunchKernelGGL(sgd_mom_f32_kernel, dim3(blocks), dim3(threads), 0,
                       stream.stream(), p.data_ptr<float>(),
                       g.data_ptr<float>(), v.data_ptr<float>(), (float)lr,
                       (float)mu, (float)wd, n);
  }
}

// All triples in ceil(count / KS_SGD_MAX_TENSORS) launches (ResNet50: 161
// tensors -> 2). grads[t] may be None: that tensor is skipped. Returns
// the number of kernels launched. G = float: f32 gradients; G = unsigned
// short: bf16 gradients, which must already have the parameter's strides.
template <typename G>
static int64_t sgd_momentum_multi_impl(
    const std::vector<torch::Tensor>& params,
    const std::vector<c10::optional<torch::Tensor>>& grads,
    const std::vector<torch::Tensor>& momenta, double lr, double mu,
    double wd) {
  constexpr bool g_f32 = std::is_same<G, float>::value;
  const auto gtype = g_f32 ? at::kFloat : at::kBFloat16;
  TORCH_CHECK(params.size() == grads.size() &&
                  params.size() == momenta.size(),
              "sgd_momentum_multi_: params, grads and momenta differ in "
              "length");
  auto stream = at::cuda::getCurrentCUDAStream();
  const long long max_blocks = 1LL << 30;
  SgdMultiArgs<G> a = {};
  a.lr = (float)lr;
  a.mu = (float)mu;
  a.wd = (float)wd;
  a.count = 0;
  a.blk[0] = 0;
  int64_t launches = 0;
  // re-strided gradient copies live until every launch is enqueued
  std::vector<torch::Tensor> keep;
  auto flush = [&]() {
    if (a.count == 0) return;
    hipLaunchKernelGGL(sgd_mom_multi_f32_kernel<G>, dim3(a.blk[a.count]),
                       dim3(KS_SGD_THREADS), 0, stream.stream(), a);
    launches++;
    a.count = 0;
  };
  for (size_t t = 0; t < params.size(); t++) {
    if (!grads[t].has_value() || !grads[t]->defined()) continue;
    auto& p = params[t];
    auto& v = momenta[t];
    torch::Tensor g = *grads[t];
    TORCH_CHECK(g.sizes() == p.sizes() && g.is_cuda() &&
                    g.scalar_type() == gtype,
                "sgd_momentum_multi_: ", g_f32 ? "f32" : "bf16",
                " CUDA gradient of the parameter's shape expected");
    if (g_f32 && g.strides() != p.strides()) {
      // rare: e.g. a contiguous gradient for a channels-last weight
      g = at::empty_like(p).copy_(g);
      keep.push_back(g);
    }
    TORCH_CHECK(p.is_cuda() && p.scalar_type() == at::kFloat &&
                    p.is_non_overlapping_and_dense() &&
                    g.sizes() == p.sizes() && g.strides() == p.strides() &&
                    v.strides() == p.strides() &&
                    g.scalar_type() == gtype &&
                    v.scalar_type() == at::kFloat,
                "sgd_momentum_: f32 dense tensors with matching strides "
                "(any memory format: the update is elementwise over the "
                "flat storage)");
    TORCH_CHECK(v.is_cuda() && v.sizes() == p.sizes() &&
                    p.get_device() == stream.device_index() &&
                    g.get_device() == p.get_device() &&
                    v.get_device() == p.get_device(),
                "sgd_momentum_multi_: parameter, gradient and momentum "
                "must live on the current device and share a shape");
    const long long n = p.numel();
    if (n == 0) continue;
    const long long nb = (n + KS_SGD_CHUNK - 1) / KS_SGD_CHUNK;
    TORCH_CHECK(nb <= max_blocks, "sgd_momentum_multi_: tensor too large");
    if (a.count == KS_SGD_MAX_TENSORS || a.blk[a.count] + nb > max_blocks)
      flush();
    a.p[a.count] = p.data_ptr<float>();
    a.g[a.count] = static_cast<const G*>(g.data_ptr());
    a.v[a.count] = v.data_ptr<float>();
    a.n[a.count] = n;
    a.blk[a.count + 1] = a.blk[a.count] + (int)nb;
    a.count++;
  }
  flush();
  return launches;
}

int64_t sgd_momentum_multi_(std::vector<torch::Tensor> params,
                            std::vector<c10::optional<torch::Tensor>> grads,
                            std::vector<torch::Tensor> momenta, double lr,
                            double mu, double wd) {
  return sgd_momentum_multi_impl<float>(params, grads, momenta, lr, mu, wd);
}

// The same update from bf16 gradients of the parameters' sizes and
// strides (a bf16 ops.GradBucket's views), upcast in registers.
int64_t sgd_momentum_multi_bf16g_(
    std::vector<torch::Tensor> params,
    std::vector<c10::optional<torch::Tensor>> grads,
    std::vector<torch::Tensor> momenta, double lr, double mu, double wd) {
  return sgd_momentum_multi_impl<unsigned short>(params, grads, momenta, lr,
                                                 mu, wd);
}

// fused NHWC bf16 BatchNorm+ReLU (bn_relu.hip)
std::vector<torch::Tensor> bn_relu_fwd_train(
    torch::Tensor x, torch::Tensor weight, torch::Tensor bias,
    torch::Tensor running_mean, torch::Tensor running_var, double momentum,
    double eps, c10::optional<torch::Tensor> res, bool relu,
    bool legacy_reduce, bool want_mask);
torch::Tensor bn_relu_fwd_eval(torch::Tensor x, torch::Tensor weight,
                               torch::Tensor bias, torch::Tensor rmean,
                               torch::Tensor rvar, double eps,
                               c10::optional<torch::Tensor> res, bool relu);
std::vector<torch::Tensor> bn_relu_bwd(
    torch::Tensor x, c10::optional<torch::Tensor> y, torch::Tensor dy,
    torch::Tensor weight, torch::Tensor bias, torch::Tensor mean,
    torch::Tensor invstd, bool need_dres, bool relu,
    c10::optional<torch::Tensor> dy2, bool legacy_reduce,
    c10::optional<torch::Tensor> mask);

// downsample BN fused into the residual join (bn_join.hip)
std::vector<torch::Tensor> bn_join_fwd_train(
    torch::Tensor x, torch::Tensor weight, torch::Tensor bias,
    torch::Tensor running_mean, torch::Tensor running_var, double momentum,
    double eps, torch::Tensor x_d, torch::Tensor weight_d,
    torch::Tensor bias_d, torch::Tensor running_mean_d,
    torch::Tensor running_var_d, double momentum_d, double eps_d,
    bool want_mask, bool legacy_reduce);
std::vector<torch::Tensor> bn_join_bwd(
    torch::Tensor x, torch::Tensor x_d, torch::Tensor y_or_mask,
    torch::Tensor dy, c10::optional<torch::Tensor> dy2, torch::Tensor weight,
    torch::Tensor weight_d, torch::Tensor mean, torch::Tensor invstd,
    torch::Tensor mean_d, torch::Tensor invstd_d, bool use_mask,
    bool legacy_reduce);

// flat gradient bucket pack / unpack (grad_bucket.hip)
int64_t grad_pack_multi(std::vector<c10::optional<torch::Tensor>> srcs,
                        torch::Tensor flat, std::vector<int64_t> offsets,
                        double scale, std::vector<torch::Tensor> like);
int64_t grad_unpack_multi(torch::Tensor flat, std::vector<int64_t> offsets,
                          std::vector<c10::optional<torch::Tensor>> dsts);

// multi-tensor f32 <-> bf16 casts (cast.hip)
std::vector<c10::optional<torch::Tensor>> cast_f32_to_bf16_multi(
    std::vector<c10::optional<torch::Tensor>> src);
std::vector<c10::optional<torch::Tensor>> cast_bf16_to_f32_multi(
    std::vector<c10::optional<torch::Tensor>> src);
// mirrored bf16 conv weights, one launch per list (cast.hip)
std::vector<torch::Tensor> mirror_weights_multi(
    std::vector<torch::Tensor> src);

// fused NHWC bf16 max-pool, one-byte argmax + gather backward (pool.hip)
std::vector<torch::Tensor> max_pool_nhwc_fwd(torch::Tensor x, int64_t k,
                                             int64_t s, int64_t p,
                                             bool want_idx);
torch::Tensor max_pool_nhwc_bwd(torch::Tensor dy, torch::Tensor idx,
                                std::vector<int64_t> input_sizes, int64_t k,
                                int64_t s, int64_t p);

// fused NHWC bf16 BN+ReLU+max-pool, recomputing backward (bn_pool.hip)
std::vector<torch::Tensor> bn_relu_pool_fwd_train(
    torch::Tensor x, torch::Tensor weight, torch::Tensor bias,
    torch::Tensor running_mean, torch::Tensor running_var, double momentum,
    double eps, int64_t k, int64_t s, int64_t p, bool want_idx,
    bool legacy_reduce);
std::vector<torch::Tensor> bn_relu_pool_fwd_eval(
    torch::Tensor x, torch::Tensor weight, torch::Tensor bias,
    torch::Tensor rmean, torch::Tensor rvar, double eps, int64_t k,
    int64_t s, int64_t p);
std::vector<torch::Tensor> bn_relu_pool_bwd(
    torch::Tensor x, torch::Tensor dy, torch::Tensor idx,
    torch::Tensor weight, torch::Tensor bias, torch::Tensor mean,
    torch::Tensor invstd, int64_t k, int64_t s, int64_t p,
    bool legacy_reduce);

// fused NHWC bf16 bias+ReLU(+max-pool) (bias_relu.hip)
torch::Tensor bias_relu_fwd(torch::Tensor x, torch::Tensor bias);
std::vector<torch::Tensor> bias_relu_bwd(torch::Tensor dy, torch::Tensor y);
std::vector<torch::Tensor> bias_relu_pool_fwd(torch::Tensor x,
                                              torch::Tensor bias, int64_t k,
                                              int64_t s, int64_t p,
                                              bool want_idx);
std::vector<torch::Tensor> bias_relu_pool_bwd(
    torch::Tensor dy, torch::Tensor idx, torch::Tensor y,
    std::vector<int64_t> input_sizes, int64_t k, int64_t s, int64_t p);

// convolution whose backward runs the weight gradient on a side stream
// (conv_split.hip)
torch::Tensor conv2d_split(torch::Tensor x, torch::Tensor w,
                           std::vector<int64_t> stride,
                           std::vector<int64_t> padding,
                           std::vector<int64_t> dilation, int64_t groups,
                           c10::optional<torch::Tensor> mirror);
void wgrad_join();
bool wgrad_pending();

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("burn", &burn, "occupy the GPU for ~ms milliseconds",
        py::arg("ms"), py::arg("blocks") = 1024, py::arg("threads") = 256);
  m.def("sgd_momentum_", &sgd_momentum_,
        "fused SGD+momentum update (in-place)");
  m.def("sgd_momentum_multi_", &sgd_momentum_multi_,
        "fused SGD+momentum update of all tensors in as few launches as "
        "the kernel-argument limit allows; a None gradient skips its "
        "tensor; returns the number of launches");
  m.def("sgd_momentum_multi_bf16g_", &sgd_momentum_multi_bf16g_,
        "sgd_momentum_multi_ reading bf16 gradients that have the "
        "parameters' sizes and strides");
  m.def("grad_pack_multi", &grad_pack_multi, py::arg("srcs"),
        py::arg("flat"), py::arg("offsets"), py::arg("scale"),
        py::arg("like"),
        "flat[offsets[t] + i] = (f32(scale) * srcs[t][i]).to(flat.dtype) "
        "over the storage of like[t]'s layout; None writes zeros; returns "
        "the number of launches");
  m.def("grad_unpack_multi", &grad_unpack_multi, py::arg("flat"),
        py::arg("offsets"), py::arg("dsts"),
        "dsts[t][i] = float(flat[offsets[t] + i]) over dsts[t]'s dense "
        "storage; None is skipped; returns the number of launches");
  m.def("bn_relu_fwd_train", &bn_relu_fwd_train, py::arg("x"),
        py::arg("weight"), py::arg("bias"), py::arg("running_mean"),
        py::arg("running_var"), py::arg("momentum"), py::arg("eps"),
        py::arg("res"), py::arg("relu"), py::arg("legacy_reduce") = false,
        py::arg("want_mask") = false,
        "{y, mean, invstd} and, with want_mask (res and relu only), the "
        "uint8 (N, H, W, C/8) ReLU mask");
  m.def("bn_relu_fwd_eval", &bn_relu_fwd_eval);
  m.def("bn_relu_bwd", &bn_relu_bwd, py::arg("x"), py::arg("y"),
        py::arg("dy"), py::arg("weight"), py::arg("bias"), py::arg("mean"),
        py::arg("invstd"), py::arg("need_dres"), py::arg("relu"),
        py::arg("dy2") = py::none(), py::arg("legacy_reduce") = false,
        py::arg("mask") = py::none(),
        "{dx, dscale, dbias[, dres]}; with mask (residual BNs) y may be "
        "None");
  m.def("bn_join_fwd_train", &bn_join_fwd_train, py::arg("x"),
        py::arg("weight"), py::arg("bias"), py::arg("running_mean"),
        py::arg("running_var"), py::arg("momentum"), py::arg("eps"),
        py::arg("x_d"), py::arg("weight_d"), py::arg("bias_d"),
        py::arg("running_mean_d"), py::arg("running_var_d"),
        py::arg("momentum_d"), py::arg("eps_d"), py::arg("want_mask"),
        py::arg("legacy_reduce") = false,
        "relu(bn(x) + bn_d(x_d)): {y, mean, invstd, mean_d, invstd_d} and, "
        "with want_mask, the uint8 (N, H, W, C/8) ReLU mask");
  m.def("bn_join_bwd", &bn_join_bwd, py::arg("x"), py::arg("x_d"),
        py::arg("y_or_mask"), py::arg("dy"), py::arg("dy2"),
        py::arg("weight"), py::arg("weight_d"), py::arg("mean"),
        py::arg("invstd"), py::arg("mean_d"), py::arg("invstd_d"),
        py::arg("use_mask"), py::arg("legacy_reduce") = false,
        "{dx, dx_d, dscale, dbias, dscale_d}; dbias serves both BNs");
  m.def("cast_f32_to_bf16_multi", &cast_f32_to_bf16_multi,
        "f32 -> bf16 (torch rounding) of every tensor of a list in as few "
        "launches as the kernel-argument limit allows; None stays None");
  m.def("cast_bf16_to_f32_multi", &cast_bf16_to_f32_multi,
        "bf16 -> f32 of every tensor of a list; None stays None");
  m.def("mirror_weights_multi", &mirror_weights_multi,
        "bf16 (K,C,R,S) weights -> new channels-last (C,K,R,S) tensors "
        "with out[c,k,r,s] = in[k,c,R-1-r,S-1-s], one launch per list");
  m.def("max_pool_nhwc_fwd", &max_pool_nhwc_fwd);
  m.def("max_pool_nhwc_bwd", &max_pool_nhwc_bwd);
  m.def("bn_relu_pool_fwd_train", &bn_relu_pool_fwd_train, py::arg("x"),
        py::arg("weight"), py::arg("bias"), py::arg("running_mean"),
        py::arg("running_var"), py::arg("momentum"), py::arg("eps"),
        py::arg("k"), py::arg("s"), py::arg("p"), py::arg("want_idx"),
        py::arg("legacy_reduce") = false,
        "{y, mean, invstd} and, with want_idx, the one-byte window codes");
  m.def("bn_relu_pool_fwd_eval", &bn_relu_pool_fwd_eval,
        "{y} from the running statistics; no codes");
  m.def("bn_relu_pool_bwd", &bn_relu_pool_bwd, py::arg("x"), py::arg("dy"),
        py::arg("idx"), py::arg("weight"), py::arg("bias"), py::arg("mean"),
        py::arg("invstd"), py::arg("k"), py::arg("s"), py::arg("p"),
        py::arg("legacy_reduce") = false, "{dx, dscale, dbias}");
  m.def("bias_relu_fwd", &bias_relu_fwd, py::arg("x"), py::arg("bias"),
        "y = bf16(relu(f32(x) + bias)), bias f32");
  m.def("bias_relu_bwd", &bias_relu_bwd, py::arg("dy"), py::arg("y"),
        "{dx, db}");
  m.def("bias_relu_pool_fwd", &bias_relu_pool_fwd, py::arg("x"),
        py::arg("bias"), py::arg("k"), py::arg("s"), py::arg("p"),
        py::arg("want_idx"),
        "{y} and, with want_idx, the one-byte window codes");
  m.def("bias_relu_pool_bwd", &bias_relu_pool_bwd, py::arg("dy"),
        py::arg("idx"), py::arg("y"), py::arg("input_sizes"), py::arg("k"),
        py::arg("s"), py::arg("p"), "{dx, db}");
  m.def("conv2d_split", &conv2d_split, py::arg("x"), py::arg("w"),
        py::arg("stride"), py::arg("padding"), py::arg("dilation"),
        py::arg("groups"), py::arg("mirror") = py::none(),
        "bias-free at::convolution; its backward runs the weight gradient "
        "on a side stream (join with wgrad_join) and, given the mirrored "
        "weight, the data gradient as a forward convolution");
  m.def("wgrad_join", &wgrad_join,
        "the current stream waits for every pending side-stream weight "
        "gradient; a no-op with nothing pending");
  m.def("wgrad_pending", &wgrad_pending,
        "True while a side-stream weight gradient has not been joined");
}
