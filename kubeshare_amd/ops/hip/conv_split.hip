// conv2d_split: a convolution whose backward runs the weight gradient on
// a side stream. Host code only; every kernel is MIOpen's.
//
// aten::convolution_backward runs the data gradient and the weight
// gradient back to back on one stream. For the flagship shapes MIOpen's
// weight-gradient solvers are split-K with f32 atomics, and its invoker
// wraps each of them in a zero fill of an f32 workspace and a cast of
// that workspace to bf16: two small, latency-bound kernels per weight
// that leave most of the machine idle while the next layer's BN backward
// waits behind them. Nothing on the backward's critical path reads a
// weight gradient (the only consumer is CastWeightsFn.backward, then the
// optimizer), so the backward here issues the same two ATen calls with
// the two halves of the output mask, the weight half under a guard for a
// side stream.
//
// Ordering and lifetimes ("Weight gradients on a side
// stream"):
//  - the side stream waits on an event recorded on the current stream at
//    backward entry: dy and the saved x are complete in its order by then
//  - dy and x get record_stream(side): autograd drops them when the
//    backward returns, and the allocator must not hand their blocks to
//    the current stream's next kernels while the side stream reads them
//  - dW is allocated under the side stream and gets record_stream(current)
//  - after each weight-gradient call an event is recorded on the side
//    stream and kept as pending; wgrad_join() makes the current stream
//    wait on it
//  - while the current stream is being captured into a graph nothing
//    forks: both halves stay on the current stream
//
// Given the mirrored weight Wm[c,k,r,s] = W[k,c,R-1-r,S-1-s]
// (mirror_weights_multi, cast.hip) the data half is the forward
// convolution of dy with Wm instead: for stride 1 that is the same sum,
// and MIOpen's tuned forward kernels are faster than its data-gradient
// kernels on these shapes ("Stride-1 data gradients as
// forward convolutions"). The weight half and everything above stay.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <ATen/cuda/CUDAEvent.h>
#include <c10/cuda/CUDAGraphsC10Utils.h>
#include <c10/cuda/CUDAGuard.h>
#include <c10/cuda/CUDAStream.h>

#include <cstdlib>
#include <memory>
#include <mutex>
#include <vector>

namespace {

struct WgradSide {
  c10::optional<c10::cuda::CUDAStream> stream;
  std::unique_ptr<at::cuda::CUDAEvent> fork, done;
  bool pending = false;
};

// backward runs on autograd's device thread, wgrad_join on whichever
// thread calls it
std::mutex g_mu;
std::vector<WgradSide> g_side;  // by device index

// KUBESHARE_WRW_PRIORITY: the priority asked of PyTorch's stream pool
// (0, the default, is also the lowest it offers on HIP; negative values
// are higher priorities and the pool clamps them to what it has)
int side_priority() {
  const char* v = std::getenv("KUBESHARE_WRW_PRIORITY");
  return v && v[0] ? std::atoi(v) : 0;
}

// g_mu held. One side stream per device, taken from the pool once.
WgradSide& side_for(c10::DeviceIndex dev) {
  if (g_side.size() <= (size_t)dev) g_side.resize((size_t)dev + 1);
  WgradSide& s = g_side[dev];
  if (!s.stream.has_value()) {
    s.stream = c10::cuda::getStreamFromPool(side_priority(), dev);
    s.fork = std::make_unique<at::cuda::CUDAEvent>();
    s.done = std::make_unique<at::cuda::CUDAEvent>();
  }
  return s;
}

bool capturing() {
  return c10::cuda::currentStreamCaptureStatusMayInitCtx() !=
         c10::cuda::CaptureStatus::None;
}

}  // namespace

struct Conv2dSplitFn : public torch::autograd::Function<Conv2dSplitFn> {
  static torch::Tensor forward(torch::autograd::AutogradContext* ctx,
                               torch::Tensor x, torch::Tensor w,
                               std::vector<int64_t> stride,
                               std::vector<int64_t> padding,
                               std::vector<int64_t> dilation, int64_t groups,
                               c10::optional<torch::Tensor> mirror) {
    TORCH_CHECK(x.is_cuda() && w.is_cuda() && x.dim() == 4 && w.dim() == 4,
                "conv2d_split: 4-d CUDA tensors expected");
    TORCH_CHECK(x.get_device() == w.get_device(),
                "conv2d_split: x and w on different devices");
    TORCH_CHECK(stride.size() == 2 && padding.size() == 2 &&
                    dilation.size() == 2,
                "conv2d_split: stride, padding and dilation take two ints");
    const bool routed = mirror.has_value() && mirror->defined();
    if (routed) {
      // the data gradient as a forward convolution of dy with the
      // mirrored weight: an identity only for these convolutions
      const int64_t r = w.size(2);
      TORCH_CHECK(stride[0] == 1 && stride[1] == 1 && dilation[0] == 1 &&
                      dilation[1] == 1 && groups == 1,
                  "conv2d_split: a mirrored weight needs stride 1, "
                  "dilation 1 and groups 1");
      TORCH_CHECK(w.size(3) == r && (r == 1 || r == 3) &&
                      padding[0] == (r - 1) / 2 && padding[1] == (r - 1) / 2,
                  "conv2d_split: a mirrored weight needs a 1x1 or 3x3 "
                  "kernel with \"same\" padding");
      TORCH_CHECK(x.scalar_type() == at::kBFloat16 &&
                      w.scalar_type() == at::kBFloat16 &&
                      mirror->scalar_type() == at::kBFloat16,
                  "conv2d_split: a mirrored weight needs bf16 x, w and "
                  "mirror");
      TORCH_CHECK(mirror->is_cuda() &&
                      mirror->get_device() == x.get_device() &&
                      mirror->dim() == 4 && mirror->size(0) == w.size(1) &&
                      mirror->size(1) == w.size(0) &&
                      mirror->size(2) == r && mirror->size(3) == r,
                  "conv2d_split: the mirrored weight of a (K,C,R,S) weight "
                  "is (C,K,R,S) on x's device");
      ctx->save_for_backward({x, w, *mirror});
    } else {
      ctx->save_for_backward({x, w});
    }
    ctx->saved_data["routed"] = routed;
    ctx->saved_data["stride"] = stride;
    ctx->saved_data["padding"] = padding;
    ctx->saved_data["dilation"] = dilation;
    ctx->saved_data["groups"] = groups;
    // the entry F.conv2d reaches: same backend choice, same solver lookup
    return at::convolution(x, w, c10::nullopt, stride, padding, dilation,
                           /*transposed=*/false, /*output_padding=*/{0, 0},
                           groups);
  }

  static torch::autograd::variable_list backward(
      torch::autograd::AutogradContext* ctx,
      torch::autograd::variable_list grads) {
    TORCH_CHECK(!at::GradMode::is_enabled(),
                "conv2d_split: double backward (create_graph=True) is not "
                "supported; set KUBESHARE_WRW_STREAM=0 for the stock "
                "convolution");
    const auto saved = ctx->get_saved_variables();
    const torch::Tensor& x = saved[0];
    const torch::Tensor& w = saved[1];
    const torch::Tensor& dy = grads[0];
    const auto stride = ctx->saved_data["stride"].toIntVector();
    const auto padding = ctx->saved_data["padding"].toIntVector();
    const auto dilation = ctx->saved_data["dilation"].toIntVector();
    const int64_t groups = ctx->saved_data["groups"].toInt();
    torch::Tensor dx, dw;
    const torch::autograd::variable_list none(7);
    if (!dy.defined()) return none;
    const bool need_dx = ctx->needs_input_grad(0);
    const bool need_dw = ctx->needs_input_grad(1);
    auto half = [&](bool data) {
      auto out = at::convolution_backward(
          dy, x, w, c10::nullopt, stride, padding, dilation,
          /*transposed=*/false, /*output_padding=*/{0, 0}, groups,
          {data, !data, false});
      return data ? std::get<0>(out) : std::get<1>(out);
    };
    // the data half: with a mirrored weight, the forward convolution of
    // dy with it ("same" padding: R-1-p == p); dW is half(false) either way
    const bool routed = ctx->saved_data["routed"].toBool();
    auto data_half = [&]() {
      if (!routed) return half(true);
      const torch::Tensor& wm = saved[2];
      const int64_t ph = wm.size(2) - 1 - padding[0];
      const int64_t pw = wm.size(3) - 1 - padding[1];
      const torch::Tensor g =
          dy.is_contiguous(at::MemoryFormat::ChannelsLast)
              ? dy
              : dy.contiguous(at::MemoryFormat::ChannelsLast);
      return at::convolution(g, wm, c10::nullopt, {1, 1}, {ph, pw}, {1, 1},
                             /*transposed=*/false, /*output_padding=*/{0, 0},
                             1);
    };
    const c10::DeviceIndex dev = (c10::DeviceIndex)dy.get_device();
    c10::cuda::CUDAGuard device_guard(dev);
    if (!need_dw || capturing()) {
      if (need_dx) dx = data_half();
      if (need_dw) dw = half(false);
      return {dx, dw, none[2], none[3], none[4], none[5], none[6]};
    }
    const auto cur = c10::cuda::getCurrentCUDAStream(dev);
    std::lock_guard<std::mutex> lock(g_mu);
    WgradSide& s = side_for(dev);
    const c10::cuda::CUDAStream side = *s.stream;
    // fork at entry: the data gradient below is not something the weight
    // gradient waits for
    s.fork->record(cur);
    s.fork->block(side);
    if (need_dx) dx = data_half();
    dy.record_stream(side);
    x.record_stream(side);
    {
      c10::cuda::CUDAStreamGuard stream_guard(side);
      dw = half(false);
    }
    dw.record_stream(cur);
    s.done->record(side);
    s.pending = true;
    return {dx, dw, none[2], none[3], none[4], none[5], none[6]};
  }
};

torch::Tensor conv2d_split(torch::Tensor x, torch::Tensor w,
                           std::vector<int64_t> stride,
                           std::vector<int64_t> padding,
                           std::vector<int64_t> dilation, int64_t groups,
                           c10::optional<torch::Tensor> mirror) {
  return Conv2dSplitFn::apply(x, w, stride, padding, dilation, groups,
                              mirror);
}

// Makes the current stream of every device with a pending weight
// gradient wait for it. Nothing pending: nothing happens. While the
// current stream is being captured the wait is skipped and the event
// stays pending: a graph cannot wait on eager work, and a capture
// begins with a device synchronize.
void wgrad_join() {
  std::lock_guard<std::mutex> lock(g_mu);
  for (size_t d = 0; d < g_side.size(); d++) {
    WgradSide& s = g_side[d];
    if (!s.pending) continue;
    c10::cuda::CUDAGuard device_guard((c10::DeviceIndex)d);
    if (capturing()) continue;
    s.done->block(c10::cuda::getCurrentCUDAStream((c10::DeviceIndex)d));
    s.pending = false;
  }
}

// True while some device has a weight gradient that no stream has
// joined yet (tests).
bool wgrad_pending() {
  std::lock_guard<std::mutex> lock(g_mu);
  for (const WgradSide& s : g_side)
    if (s.pending) return true;
  return false;
}
