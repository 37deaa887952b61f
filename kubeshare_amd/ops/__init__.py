"""kubeshare_amd.ops — hand-written HIP/gfx950 kernels.

Build: in-tree (the built .so travels with the repo snapshot), via
torch.utils.cpp_extension with PYTORCH_ROCM_ARCH=gfx950. On a GPU box a
missing extension is a hard error (fail-loud policy): GPU
paths must never silently fall back to eager PyTorch.
"""
from __future__ import annotations

import functools
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_BUILD_DIR = os.path.join(_HERE, "_build")
_SRCS = [os.path.join(_HERE, "hip", "ks_ops.hip"),
         os.path.join(_HERE, "hip", "bn_relu.hip"),
         os.path.join(_HERE, "hip", "pool.hip"),
         os.path.join(_HERE, "hip", "bn_pool.hip"),
         os.path.join(_HERE, "hip", "bn_join.hip"),
         os.path.join(_HERE, "hip", "bias_relu.hip"),
         os.path.join(_HERE, "hip", "cast.hip"),
         os.path.join(_HERE, "hip", "conv_split.hip"),
         os.path.join(_HERE, "hip", "grad_bucket.hip")]

_ext = None


def build_extension(verbose: bool = False):
    """Compile the extension for gfx950 (works on a CPU-only box: hipcc
    cross-compiles). Called by __graft_entry__.build()."""
    import torch  # noqa: F401  (sets up the ROCm toolchain env)
    from torch.utils import cpp_extension

    os.environ.setdefault("PYTORCH_ROCM_ARCH", "gfx950")
    os.makedirs(_BUILD_DIR, exist_ok=True)
    return cpp_extension.load(
        name="ks_ops",
        sources=_SRCS,
        build_directory=_BUILD_DIR,
        extra_cflags=["-O3"],
        verbose=verbose,
        is_python_module=True,
    )


def _load():
    global _ext
    if _ext is not None:
        return _ext
    import torch

    so = os.path.join(_BUILD_DIR, "ks_ops.so")
    if os.path.exists(so):
        import importlib.util

        spec = importlib.util.spec_from_file_location("ks_ops", so)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _ext = mod
        return _ext
    if torch.cuda.is_available():
        # GPU box without a prebuilt .so: build now — never fall back
        # silently to eager PyTorch on the GPU path.
        _ext = build_extension()
        return _ext
    raise ImportError(
        "kubeshare_amd.ops extension not built; run __graft_entry__.build()")


def burn(ms: float, blocks: int = 1024, threads: int = 256):
    """Occupy the current GPU for ~ms milliseconds (calibrated load
    generator used by the isolation tests and rocprof quota proofs)."""
    _load().burn(float(ms), blocks, threads)


class FusedSGD:
    """Multi-tensor fused SGD+momentum (f32 master params).

    Matches torch.optim.SGD(momentum=mu, weight_decay=wd, dampening=0,
    nesterov=False) semantics. step() hands every (param, grad, momentum)
    triple to ONE multi-tensor kernel launch per 110 tensors (ResNet50:
    161 tensors, 2 launches); pointers travel in the kernel arguments,
    so nothing requires the gradients to stay at the same address.

    zero_grad() therefore just drops the gradients (no kernels): the
    next backward pass adopts its freshly computed gradient tensors
    instead of running one fill and one `grad += new` kernel per
    parameter.

    graph_mode="auto" (default on CUDA): the one- or two-node step is
    still captured into a hipGraph after the first full eager step, and
    replayed only while every parameter, gradient and momentum pointer
    equals the captured one; any other step launches eagerly.

    KUBESHARE_SGD_MULTI=0 selects the per-tensor kernel (one launch per
    tensor) for A/B runs; KUBESHARE_SGD_GRAPH=0 disables the capture.

    process_group (a torch.distributed group, or True for the default
    group) makes the optimizer average the gradients over that group,
    for a model that is NOT wrapped in DistributedDataParallel. step()
    is then: wgrad_join(); pack every gradient, scaled by 1/world, into
    one persistent flat GradBucket of grad_dtype (f32 or bf16); ONE
    all-reduce of the bucket; the multi-tensor SGD with the bucket's
    views as gradients (a bf16 bucket is upcast in registers). These
    steps launch eagerly, never from a captured graph (a gloo collective
    cannot be captured), and always through the multi-tensor kernel.
    Unlike the ungrouped step, which skips a parameter whose gradient is
    None, the grouped step gives such a parameter a zero gradient and
    updates it like any other (momentum and weight decay still move it):
    every rank must all-reduce the same layout, and a rank that raised
    or skipped would leave its peers waiting. With process_group=None
    nothing of this exists and the optimizer is the ungrouped one.
    """

    def __init__(self, params, lr: float, momentum: float = 0.9,
                 weight_decay: float = 0.0, graph_mode: str = "auto",
                 process_group=None, grad_dtype=None):
        import torch

        self.params = [p for p in params if p.requires_grad]
        self._bucket = None
        if process_group is not None and process_group is not False:
            import torch.distributed as dist

            self._group = None if process_group is True else process_group
            self._world = dist.get_world_size(self._group)
            self._bucket = GradBucket(
                self.params,
                torch.float32 if grad_dtype is None else grad_dtype)
        elif grad_dtype not in (None, torch.float32):
            raise ValueError("grad_dtype needs a process_group: ungrouped "
                             "steps read the f32 gradients themselves")
        self.lr = lr
        self.momentum = momentum
        self.weight_decay = weight_decay
        # momentum buffers share the parameter's layout (channels-last
        # conv weights included): the kernel updates flat dense storage
        self.momenta = [torch.zeros_like(p) for p in self.params]
        self._graph_mode = graph_mode
        self._multi = os.environ.get("KUBESHARE_SGD_MULTI", "1") != "0"
        self._step_graph = None
        self._graph_ptrs = None  # data_ptrs the graph was baked on

    def _graphable(self):
        import torch
        if self._graph_mode == "off" or not torch.cuda.is_available():
            return False
        if os.environ.get("KUBESHARE_SGD_GRAPH", "1") == "0":
            return False
        return all(p.grad is not None and p.grad.is_cuda
                   for p in self.params)

    def _ptrs(self):
        """Every address a captured step would touch; a replay is valid
        only while all of them are what they were at capture."""
        return tuple(
            (p.data_ptr(), v.data_ptr(),
             p.grad.data_ptr() if p.grad is not None else 0)
            for p, v in zip(self.params, self.momenta))

    def zero_grad(self, set_to_none: bool = True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def _launch(self):
        ext = _load()
        if self._multi:
            ext.sgd_momentum_multi_(
                [p.data for p in self.params],
                [p.grad for p in self.params], self.momenta,
                self.lr, self.momentum, self.weight_decay)
            return
        ps, gs, vs = [], [], []
        for p, v in zip(self.params, self.momenta):
            if p.grad is None:
                continue
            ps.append(p.data)
            gs.append(p.grad)
            vs.append(v)
        ext.sgd_momentum_(ps, gs, vs, self.lr, self.momentum,
                          self.weight_decay)

    def _group_step(self):
        """Average over the group, then update from the bucket (see the
        class docstring); the side stream has been joined."""
        import torch
        bucket = self._bucket
        bucket.pack([p.grad for p in self.params], 1.0 / self._world)
        bucket.all_reduce(self._group)
        ext = _load()
        sgd = ext.sgd_momentum_multi_ if bucket.dtype == torch.float32 \
            else ext.sgd_momentum_multi_bf16g_
        sgd([p.data for p in self.params], bucket.views, self.momenta,
            self.lr, self.momentum, self.weight_decay)

    def _capture(self):
        import torch
        ptrs = self._ptrs()
        # (the update kernel is already warm: capture happens right
        # after a full eager step)
        step_g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(step_g):
            self._launch()
        self._step_graph = step_g
        self._graph_ptrs = ptrs

    def step(self):
        # torch SGD's first step sets v = g + wd*p (no mu*v term since v
        # starts at 0) — identical here because v == 0.
        # (a backward that ended early or raised never reached
        # CastWeightsFn's join: no side-stream weight gradient outlives
        # the step)
        wgrad_join()
        if self._bucket is not None:
            self._group_step()
            return
        if self._step_graph is not None and \
                self._graph_ptrs == self._ptrs():
            self._step_graph.replay()
            return
        self._launch()
        # after a full-set eager step, capture the graph; it serves the
        # later steps whose gradients land at the same addresses
        if self._step_graph is None and self._graph_mode == "auto" and \
                self._graphable():
            try:
                self._capture()
            except Exception:  # noqa: BLE001 — capture is an optimization
                self._graph_mode = "off"


# ------------------------------------------------- flat gradient bucket
def _dense(t) -> bool:
    """Non-overlapping and dense: t's elements fill numel() consecutive
    storage slots in some dimension order (contiguous, channels-last,
    any permutation of a contiguous tensor)."""
    expect = 1
    for size, stride in sorted(
            ((s, st) for s, st in zip(t.size(), t.stride()) if s != 1),
            key=lambda d: d[1]):
        if size == 0:
            return True
        if stride != expect:
            return False
        expect *= size
    return True


class GradBucket:
    """One persistent flat buffer with a segment per tensor of `params`
    (f32 tensors on one device), of dtype f32 or bf16: what a gang rank
    all-reduces in ONE collective (FusedSGD(process_group=...)) or
    broadcasts (broadcast_parameters).

    Segment t starts at offsets[t], a multiple of 8 elements (16 bytes
    in bf16, 32 in f32, so every segment takes the kernels' 16-byte
    vector path), and holds the tensor's flat dense storage in storage
    order; the padding between segments is zeroed here and never written
    again. views[t] = flat.as_strided(p.size(), p.stride(), offsets[t]):
    the segment seen with the parameter's sizes and strides, which is
    what the multi-tensor SGD takes as a gradient. Parameters must be
    non-overlapping and dense (ValueError otherwise).

    pack(tensors, scale) writes view_t = (tensor_t * f32(scale)).to(dtype)
    and zeros for a None entry; unpack(tensors) writes tensor_t =
    view_t.float(). On CUDA both run hip/grad_bucket.hip (up to 128
    tensors per launch) and nothing else: no eager fall-back. On CPU
    tensors they run exactly those torch expressions, so the layout
    logic is testable without a GPU."""

    ALIGN = 8  # elements

    def __init__(self, params, dtype=None):
        import torch

        self.params = list(params)
        self.dtype = torch.float32 if dtype is None else dtype
        if self.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("GradBucket: dtype must be float32 or "
                             f"bfloat16, not {self.dtype}")
        device = self.params[0].device if self.params else "cpu"
        self.offsets = []
        end = 0
        for p in self.params:
            if p.dtype != torch.float32 or p.device != device:
                raise ValueError("GradBucket: f32 tensors on one device "
                                 "expected")
            if not _dense(p):
                raise ValueError(
                    "GradBucket: parameters must be non-overlapping and "
                    f"dense, got sizes {tuple(p.size())} strides "
                    f"{tuple(p.stride())}")
            self.offsets.append(end)
            end += p.numel()
            end += -end % self.ALIGN
        self.flat = torch.zeros(end, dtype=self.dtype, device=device)
        self.views = [self.flat.as_strided(p.size(), p.stride(), off)
                      for p, off in zip(self.params, self.offsets)]

    def _check(self, tensors):
        tensors = list(tensors)
        if len(tensors) != len(self.views):
            raise ValueError(f"GradBucket: {len(self.views)} tensors "
                             f"expected, got {len(tensors)}")
        return tensors

    def pack(self, tensors, scale: float = 1.0):
        """view_t = (tensor_t * scale).to(dtype), zeros for None. The
        scale is rounded to f32 once, here; the product is one f32
        multiply per element. A tensor whose strides differ from its
        parameter's (a contiguous gradient for a channels-last weight)
        is re-strided first."""
        import torch

        tensors = self._check(tensors)
        scale = torch.tensor(scale, dtype=torch.float32).item()
        if self.flat.is_cuda:
            _load().grad_pack_multi(tensors, self.flat, self.offsets, scale,
                                    self.views)
            return
        with torch.no_grad():
            for view, g in zip(self.views, tensors):
                if g is None:
                    view.zero_()
                else:
                    view.copy_((g * scale).to(self.dtype))

    def unpack(self, tensors):
        """tensor_t = view_t.float(), in place; None entries are
        skipped. Every tensor must have its parameter's sizes and
        strides."""
        import torch

        tensors = self._check(tensors)
        for view, t in zip(self.views, tensors):
            if t is not None and (t.size() != view.size()
                                  or t.stride() != view.stride()):
                raise ValueError("GradBucket.unpack: destination with the "
                                 "parameter's sizes and strides expected")
        if self.flat.is_cuda:
            _load().grad_unpack_multi(self.flat, self.offsets, tensors)
            return
        with torch.no_grad():
            for view, t in zip(self.views, tensors):
                if t is not None:
                    t.copy_(view.float())

    def all_reduce(self, group=None):
        """Sum the flat buffer over the group (None: the default
        group), in place; the caller's pack() scale makes it a mean."""
        import torch.distributed as dist

        dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=group)


def broadcast_parameters(model, src: int = 0, group=None):
    """Give every rank of the group rank `src`'s parameters and
    floating-point buffers (BN running statistics): all of them are
    packed into a temporary f32 GradBucket, sent by ONE broadcast and
    unpacked in place. Call it once, before training, on a model that is
    not wrapped in DistributedDataParallel. `src` is a global rank.

    Nothing synchronises the buffers afterwards: BN running statistics
    are local to a rank (each follows its own batches), exactly as under
    DistributedDataParallel(broadcast_buffers=False). Integer buffers
    (num_batches_tracked) are left alone. Tensors must be f32."""
    import torch
    import torch.distributed as dist

    tensors = [p.data for p in model.parameters()]
    tensors += [b for b in model.buffers() if b.is_floating_point()]
    with torch.no_grad():
        bucket = GradBucket(tensors, torch.float32)
        bucket.pack(tensors)
        dist.broadcast(bucket.flat, src=src, group=group)
        bucket.unpack(tensors)


# ---------------------------------------------- shared NHWC predicates
def _nhwc_bf16_ok(x, min_c=0, max_pixels=None) -> bool:
    """What every fused NHWC kernel needs of an activation: 4-D, on the
    GPU, bf16, channels-last, C % 8 == 0 and min_c <= C <= 2048 (a block
    spans a pixel's channel groups); with max_pixels also N*H*W below it
    (the kernels that split a pixel index into (n, h, w) keep it in 32
    bits). The public *_supported functions add what is their own."""
    import torch

    if x.dim() != 4:
        return False
    n, c, h, w = x.shape
    return (x.is_cuda and x.dtype == torch.bfloat16
            and c % 8 == 0 and min_c <= c <= 2048
            and (max_pixels is None or n * h * w < max_pixels)
            and x.is_contiguous(memory_format=torch.channels_last))


def _channels_last(dy):
    """dy as the kernels read it: y.sum().backward() hands over a
    stride-0 expanded gradient, and autograd promises no layout."""
    import torch

    if dy.is_contiguous(memory_format=torch.channels_last):
        return dy
    return dy.contiguous(memory_format=torch.channels_last)


# ---------------------------------------------------- fused BN+ReLU(+add)
@functools.lru_cache(maxsize=None)
def _bn_relu_autograd():
    """Build the autograd.Function once (torch import deferred)."""
    import torch

    class BNReLUFn(torch.autograd.Function):
        """y = relu(batch_norm(x) [+ res]) on NHWC bf16 via the gfx950
        kernels in hip/bn_relu.hip. Replaces MIOpen's 5-pass forward /
        8-pass backward (incl. separate ReLU and residual-add kernels)
        with 3 forward passes and 5 (non-residual, mask recomputed
        from x) / 7 (residual, dym reuse) backward passes — see
        profiles/README.md for the motivation. Each direction is three
        launches: stats, one coalesced reduce of the block partials
        (which in forward also finalizes mean/invstd, the running stats
        and the folded scale/bias), apply. KUBESHARE_BN_REDUCE=legacy
        (see bn_reduce_legacy) runs the earlier reduce and finalize
        kernels instead; both compute the same bits.

        fork=True returns the pair (y, y2) with y2 = y.view_as(y): the
        same memory under two autograd edges, one per consumer of a
        residual join (the next block's conv1 and its identity branch).
        The backward then receives the two gradients separately and the
        stats kernel sums them in registers, instead of autograd running
        a separate bf16 add kernel whose result that kernel re-reads.
        Nothing on the fused path writes in place into y or y2; an
        in-place op on either would corrupt the other consumer's input,
        so keep it that way.

        A residual BN in training mode saves the ReLU mask as bits (one
        byte per 8 channels, written by the forward apply kernel)
        instead of y: its backward stats kernel then reads 1/16 of a
        pass where it read a whole one, for the same bits out.
        KUBESHARE_BN_MASK=0 (see bn_mask_enabled) keeps y."""

        @staticmethod
        def forward(ctx, x, res, weight, bias, running_mean, running_var,
                    training, momentum, eps, relu, fork=False):
            ext = _load()
            w32 = weight.float()
            b32 = bias.float()
            # backward takes undefined gradients as None (a forked
            # output may have no consumer) instead of zero tensors
            ctx.set_materialize_grads(False)
            ctx.with_res = res is not None
            ctx.relu = relu
            ctx.wdtype = weight.dtype
            ctx.legacy_reduce = bn_reduce_legacy()
            ctx.masked = bool(training and relu and res is not None
                              and bn_mask_enabled())
            if training:
                out = ext.bn_relu_fwd_train(
                    x, w32, b32, running_mean, running_var, momentum, eps,
                    res, relu, ctx.legacy_reduce, ctx.masked)
                y, mean, invstd = out[0], out[1], out[2]
                ctx.save_for_backward(x, out[3] if ctx.masked else y, w32,
                                      b32, mean, invstd)
            else:
                y = ext.bn_relu_fwd_eval(x, w32, b32, running_mean.float(),
                                         running_var.float(), eps, res, relu)
                ctx.save_for_backward(x, y, w32, b32, running_mean.float(),
                                      (running_var.float() + eps).rsqrt())
            return (y, y.view_as(y)) if fork else y

        @staticmethod
        def backward(ctx, dy, dy2=None):
            ext = _load()
            x, y, w32, b32, mean, invstd = ctx.saved_tensors
            if dy is None:
                dy, dy2 = dy2, None
            if dy is None:  # no gradient reached either output
                return (None,) * 11
            # y is the ReLU mask (uint8) when ctx.masked
            out = ext.bn_relu_bwd(x, None if ctx.masked else y, dy, w32,
                                  b32, mean, invstd, ctx.with_res, ctx.relu,
                                  dy2, ctx.legacy_reduce,
                                  y if ctx.masked else None)
            dx, dscale, dbias = out[0], out[1], out[2]
            dres = out[3] if ctx.with_res else None
            return (dx, dres, dscale.to(ctx.wdtype), dbias.to(ctx.wdtype),
                    None, None, None, None, None, None, None)

    return BNReLUFn


def bn_fork_enabled() -> bool:
    """KUBESHARE_BN_FORK=0 keeps the residual joins unforked (autograd
    sums the two gradients with its own add kernel); A/B runs, operator
    escape hatch."""
    return os.environ.get("KUBESHARE_BN_FORK", "1") != "0"


def bn_reduce_legacy() -> bool:
    """KUBESHARE_BN_REDUCE=legacy reduces the BN block partials with the
    earlier one-wave-per-channel kernel and, in forward, a separate
    finalize launch, instead of the coalesced reduce(+finalize) kernel.
    Same results bit for bit; A/B runs and the oracle of
    tests/test_bn_reduce_gpu.py."""
    return os.environ.get("KUBESHARE_BN_REDUCE", "") == "legacy"


def bn_mask_enabled() -> bool:
    """KUBESHARE_BN_MASK=0 makes the residual BNs (BNReLUFn with res,
    BNJoinFn) save y for their backward instead of the one-byte-per-8-
    channels ReLU mask. Same results bit for bit; A/B runs and the
    oracle of tests/test_bn_mask_gpu.py."""
    return os.environ.get("KUBESHARE_BN_MASK", "1") != "0"


def bn_relu(x, bn, res=None, relu=True, fork=False):
    """Fused BN[+ReLU][+residual add] using an nn.BatchNorm2d's
    parameters/buffers; relu=False serves activation-free BNs (the
    ResNet downsample path). Falls back to eager for shapes the kernel
    does not cover (non-bf16, C%8!=0, not channels-last).

    fork=True returns the pair (y, y2), one handle per consumer of a
    residual join (see BNReLUFn); the eager fall-back returns (y, y)."""
    import torch

    supported = _nhwc_bf16_ok(x)
    if supported and res is not None and res.dtype != torch.bfloat16:
        # downsample-path BN runs in fp32 under autocast; the residual
        # join is bf16 in bf16 training
        res = res.to(torch.bfloat16)
    if not supported:
        y = torch.nn.functional.batch_norm(
            x, bn.running_mean, bn.running_var, bn.weight, bn.bias,
            bn.training, bn.momentum, bn.eps)
        if res is not None:
            y = y + res
        y = torch.relu(y) if relu else y
        return (y, y) if fork else y
    if res is not None and not res.is_contiguous(
            memory_format=torch.channels_last):
        res = res.contiguous(memory_format=torch.channels_last)
    fn = _bn_relu_autograd()
    return fn.apply(x, res, bn.weight, bn.bias, bn.running_mean,
                    bn.running_var, bn.training, bn.momentum, bn.eps, relu,
                    fork)


# ------------------------- downsample BN fused into the residual join
def bn_join_enabled() -> bool:
    """KUBESHARE_BN_JOIN=0 runs a downsample block's join as the two ops
    bn_relu(x, bn, res=bn_relu(x_d, bn_d, relu=False)) wherever bn_join
    would have fused them (A/B runs, operator escape hatch)."""
    return os.environ.get("KUBESHARE_BN_JOIN", "1") != "0"


@functools.lru_cache(maxsize=None)
def _bn_join_autograd():
    """Build the autograd.Function once (torch import deferred)."""
    import torch

    class BNJoinFn(torch.autograd.Function):
        """y = relu(bn(x) + bn_d(x_d)) on NHWC bf16, training mode, via
        hip/bn_join.hip: the downsample BN's output is never allocated
        and the backward runs one stats and one apply kernel for both
        BNs. Values and gradients are those of BNReLUFn(x, res=
        BNReLUFn(x_d, relu=False)), bit for bit; the bias gradient of
        the two BNs is one sum. fork and the saved ReLU mask are
        BNReLUFn's."""

        @staticmethod
        def forward(ctx, x, x_d, weight, bias, running_mean, running_var,
                    momentum, eps, weight_d, bias_d, running_mean_d,
                    running_var_d, momentum_d, eps_d, fork):
            ext = _load()
            w32, b32 = weight.float(), bias.float()
            wd32, bd32 = weight_d.float(), bias_d.float()
            ctx.set_materialize_grads(False)
            ctx.wdtype = weight.dtype
            ctx.wdtype_d = weight_d.dtype
            ctx.legacy_reduce = bn_reduce_legacy()
            ctx.masked = bn_mask_enabled()
            out = ext.bn_join_fwd_train(
                x, w32, b32, running_mean, running_var, momentum, eps,
                x_d, wd32, bd32, running_mean_d, running_var_d, momentum_d,
                eps_d, ctx.masked, ctx.legacy_reduce)
            y = out[0]
            ctx.save_for_backward(x, x_d, out[5] if ctx.masked else y, w32,
                                  wd32, *out[1:5])
            return (y, y.view_as(y)) if fork else y

        @staticmethod
        def backward(ctx, dy, dy2=None):
            x, x_d, ym, w32, wd32, mean, invstd, mean_d, invstd_d = \
                ctx.saved_tensors
            if dy is None:
                dy, dy2 = dy2, None
            if dy is None:  # no gradient reached either output
                return (None,) * 15
            dx, dx_d, dscale, dbias, dscale_d = _load().bn_join_bwd(
                x, x_d, ym, dy, dy2, w32, wd32, mean, invstd, mean_d,
                invstd_d, ctx.masked, ctx.legacy_reduce)
            # one sum, two parameters: each gets a tensor of its own
            return (dx, dx_d, dscale.to(ctx.wdtype), dbias.to(ctx.wdtype),
                    None, None, None, None, dscale_d.to(ctx.wdtype_d),
                    dbias.clone().to(ctx.wdtype_d), None, None, None, None,
                    None)

    return BNJoinFn


def bn_join_supported(x, x_d) -> bool:
    """True when hip/bn_join.hip covers the pair: both channels-last bf16
    on the GPU, of one shape, C % 8 == 0 and C <= 2048."""
    return (x.shape == x_d.shape and _nhwc_bf16_ok(x)
            and _nhwc_bf16_ok(x_d))


def bn_join(x, bn, x_d, bn_d, fork=False):
    """relu(bn(x) + bn_d(x_d)): the residual join of a downsample block
    (x the block's last conv output, x_d the downsample conv's) as one
    fused op (hip/bn_join.hip), using the two nn.BatchNorm2d's
    parameters and buffers exactly as bn_relu does. Outside
    bn_join_supported, unless both BNs are in training mode, and under
    KUBESHARE_BN_JOIN=0 it runs the composition
    bn_relu(x, bn, res=bn_relu(x_d, bn_d, relu=False), fork=fork), which
    has its own eager fall-backs. fork is bn_relu's."""
    if not (bn_join_enabled() and bn.training and bn_d.training
            and bn_join_supported(x, x_d)):
        return bn_relu(x, bn, res=bn_relu(x_d, bn_d, relu=False), fork=fork)
    fn = _bn_join_autograd()
    return fn.apply(x, x_d, bn.weight, bn.bias, bn.running_mean,
                    bn.running_var, bn.momentum, bn.eps, bn_d.weight,
                    bn_d.bias, bn_d.running_mean, bn_d.running_var,
                    bn_d.momentum, bn_d.eps, fork)


# ------------------------------------------- multi-tensor weight casts
@functools.lru_cache(maxsize=None)
def _cast_weights_autograd():
    """Build the autograd.Function once (torch import deferred)."""
    import torch

    class CastWeightsFn(torch.autograd.Function):
        """(w0, w1, ...) f32 -> (bf16 copies) in one multi-tensor launch
        of hip/cast.hip per 128 tensors, strides preserved; the backward
        casts the incoming bf16 gradients back to f32 the same way. A
        gradient that is already f32, or None, passes through untouched.
        The backward first joins the weight-gradient side stream
        (wgrad_join): autograd runs this node once every staged weight's
        gradient has been issued, and it is their first reader.
        Values are exactly those of w.to(torch.bfloat16) and g.float():
        this replaces autocast's per-weight cast launches and their
        ToCopyBackward0 nodes, nothing else."""

        @staticmethod
        def forward(ctx, *weights):
            ctx.set_materialize_grads(False)
            return tuple(_load().cast_f32_to_bf16_multi(list(weights)))

        @staticmethod
        def backward(ctx, *grads):
            wgrad_join()
            out = list(grads)
            idx = [i for i, g in enumerate(grads)
                   if g is not None and g.dtype == torch.bfloat16]
            if idx:
                cast = _load().cast_bf16_to_f32_multi(
                    [grads[i] for i in idx])
                for i, g in zip(idx, cast):
                    out[i] = g
            return tuple(out)

    return CastWeightsFn


def cast_weights_bf16(weights):
    """bf16 copies of a sequence of f32 CUDA tensors through
    CastWeightsFn (differentiable; works under no_grad and inside a
    hipGraph capture: addresses ride in the kernel arguments)."""
    fn = _cast_weights_autograd()
    return fn.apply(*weights)


def lowp_weights_enabled() -> bool:
    """KUBESHARE_LOWP_WEIGHTS=0 leaves every conv weight to autocast's
    own per-tensor cast (A/B runs, operator escape hatch)."""
    return os.environ.get("KUBESHARE_LOWP_WEIGHTS", "1") != "0"


def stage_lowp_weights(convs):
    """Give every models.conv.LowpConv2d in `convs` a bf16 copy of its
    weight for the forward in progress, all cast by one launch. Happens
    only under CUDA autocast with dtype bf16, for f32 CUDA weights, and
    unless KUBESHARE_LOWP_WEIGHTS=0; otherwise nothing is staged and the
    convs use self.weight as ever. Returns the modules staged, for
    clear_lowp_weights."""
    import torch

    if not convs or not lowp_weights_enabled():
        return []
    if not torch.is_autocast_enabled("cuda") or \
            torch.get_autocast_dtype("cuda") != torch.bfloat16:
        return []
    weights = [m.weight for m in convs]
    if not all(w.is_cuda and w.dtype == torch.float32 for w in weights):
        return []
    wgrad_join()  # nothing of an abandoned backward runs into this step
    for m, w in zip(convs, cast_weights_bf16(weights)):
        m._lowp_weight = w
    # one more launch mirrors the staged weight of every conv flagged by
    # fuse_model (see dgrad_fwd_mode), for conv2d_split's data gradient
    if torch.is_grad_enabled() and dgrad_fwd_active():
        flagged = [m for m in convs if getattr(m, "_dgrad_fwd", False)
                   and m.weight.requires_grad]
        if flagged:
            mirrors = _load().mirror_weights_multi(
                [m._lowp_weight.detach() for m in flagged])
            for m, wm in zip(flagged, mirrors):
                m._lowp_mirror = wm
    return convs


def clear_lowp_weights(convs):
    """Drop the staged copies (the autograd graph keeps what it needs)."""
    for m in convs:
        m._lowp_weight = None
        m._lowp_mirror = None


# ----------------- stride-1 data gradients as forward convolutions
_DGRAD_FWD_MODES = ("0", "1x1", "3x3", "all", "")


def dgrad_fwd_mode() -> str:
    """KUBESHARE_DGRAD_FWD selects which convs of a fused model run their
    data gradient as a forward convolution of dy with the mirrored
    weight (conv2d_split(mirror=...)): unset, every eligible 1x1 and 3x3
    conv whose mirrored forward shape the model also runs as a forward
    (see dgrad_fwd_flags); `1x1` or `3x3`, only that class under the
    same rule; `all`, every eligible conv whatever the model contains;
    `0`, none: no mirror launch, the stock data gradient (A/B runs,
    operator escape hatch). fuse_model reads it when it flags the convs;
    `0` is also honoured at every forward, and so is
    torch.backends.cudnn.deterministic while the switch is unset
    (dgrad_fwd_active)."""
    v = os.environ.get("KUBESHARE_DGRAD_FWD", "")
    if v not in _DGRAD_FWD_MODES:
        raise ValueError(f"KUBESHARE_DGRAD_FWD={v!r}: one of 0, 1x1, 3x3, "
                         "all expected")
    return v


def dgrad_fwd_active() -> bool:
    """Whether stage_lowp_weights mirrors the flagged convs' weights for
    the forward in progress: not under KUBESHARE_DGRAD_FWD=0, and, with
    the switch unset, not while torch.backends.cudnn.deterministic is
    set. The routing rests on a measurement: MIOpen's tuned forward
    solvers beat its tuned data-gradient solvers on these shapes. With
    the deterministic attribute MIOpen chooses among other solvers, for
    which nothing was measured, and whoever sets it is comparing values
    between runs or code paths (tests/test_lowp_weights_gpu.py holds
    staged against unstaged BN gradients bitwise that way), which a dx
    summed in another order would break for no known gain. An explicit
    KUBESHARE_DGRAD_FWD=1x1, 3x3 or all routes regardless."""
    import torch

    mode = dgrad_fwd_mode()
    if mode == "0":
        return False
    return mode != "" or not torch.backends.cudnn.deterministic


def _dgrad_fwd_signature(m):
    """(in, out, k) of a conv whose data gradient is a forward
    convolution with the mirrored weight and that conv2d_split accepts
    with one: stride 1, dilation 1, groups 1, a 1x1 or 3x3 kernel with
    "same" zero padding, no bias. None for any other module."""
    import torch.nn as nn

    if not isinstance(m, nn.Conv2d) or m.bias is not None \
            or m.padding_mode != "zeros" or isinstance(m.padding, str):
        return None
    k = m.kernel_size[0]
    if tuple(m.kernel_size) != (k, k) or k not in (1, 3) \
            or tuple(m.stride) != (1, 1) or tuple(m.dilation) != (1, 1) \
            or m.groups != 1 or tuple(m.padding) != (k // 2, k // 2):
        return None
    return (m.in_channels, m.out_channels, k)


def dgrad_fwd_flags(model, mode=None):
    """{LowpConv2d: bool} for every LowpConv2d of `model`: whether its
    data gradient is to run as a forward convolution under `mode`
    (default: dgrad_fwd_mode()). A conv qualifies when it has a
    _dgrad_fwd_signature and, except under `all`, the model also
    contains a conv with the mirrored signature (in and out swapped,
    same kernel): the mirrored forward is then a shape the model runs as
    a forward anyway, which is the structural stand-in for "the tuned
    MIOpen db has that forward shape". For ResNet50 that is 43 of the 53
    convs; layer{2,3,4}.0.conv1 (forward shapes 128->256 @56, 256->512
    @28, 512->1024 @14 are in no db), the stride-2 convs and the stem
    stay on the stock data gradient."""
    from ..models.conv import LowpConv2d

    mode = dgrad_fwd_mode() if mode is None else mode
    sigs = {m: _dgrad_fwd_signature(m) for m in model.modules()}
    present = {s for s in sigs.values() if s is not None}
    flags = {}
    for m, sig in sigs.items():
        if not isinstance(m, LowpConv2d):
            continue
        ok = sig is not None and mode != "0"
        if ok and mode in ("1x1", "3x3"):
            ok = mode == f"{sig[2]}x{sig[2]}"
        if ok and mode != "all":
            ok = (sig[1], sig[0], sig[2]) in present
        flags[m] = ok
    return flags


# ------------------------------ conv weight gradients on a side stream
def wrw_stream_enabled() -> bool:
    """KUBESHARE_WRW_STREAM=0 keeps every models.conv.LowpConv2d on the
    stock convolution, whose backward runs the data gradient and the
    weight gradient back to back on one stream, instead of
    conv2d_split (A/B runs, operator escape hatch).
    KUBESHARE_WRW_PRIORITY=<int> (read once, when the side stream is
    taken) asks PyTorch's stream pool for that priority: 0, the default,
    is also the lowest the pool offers on HIP, -1 the high-priority
    pool."""
    return os.environ.get("KUBESHARE_WRW_STREAM", "1") != "0"


def conv2d_split(x, w, stride=(1, 1), padding=(0, 0), dilation=(1, 1),
                 groups=1, mirror=None):
    """Bias-free F.conv2d(x, w, None, stride, padding, dilation, groups)
    for CUDA tensors through hip/conv_split.hip: same ATen entry, same
    MIOpen kernels, same values, but the backward issues the weight
    gradient on a side stream (one per device), where MIOpen's zero-fill
    and cast kernels around each split-K weight-gradient kernel run
    beside the main stream's kernels instead of between them. The
    returned dW is NOT ordered with the stream that called backward()
    until wgrad_join() has run on that stream: CastWeightsFn.backward,
    FusedSGD.step and stage_lowp_weights call it, and any other reader
    must. Inside a graph capture the backward does not fork. Double
    backward raises.

    mirror: optionally the mirrored weight, (C,K,R,S) with
    mirror[c,k,r,s] = w[k,c,R-1-r,S-1-s] (mirror_weights), not
    differentiated. The backward then computes dx as the forward
    convolution of dy with it, where MIOpen's forward kernels beat its
    data-gradient kernels, instead of convolution_backward's data half.
    Accepted only for bf16, stride 1, dilation 1, groups 1 and a 1x1 or
    3x3 kernel with "same" padding; anything else raises."""
    def two(v):
        return [int(v), int(v)] if isinstance(v, int) else [int(i) for i in v]
    return _load().conv2d_split(x, w, two(stride), two(padding),
                                two(dilation), int(groups), mirror)


def mirror_weights(weights):
    """For each bf16 CUDA weight (K,C,R,S) of the list a new channels-last
    (C,K,R,S) tensor with out[c,k,r,s] = in[k,c,R-1-r,S-1-s], all by one
    launch of hip/cast.hip per 127 tensors (capturable: addresses ride in
    the kernel arguments). A tensor that is not dense channels-last bf16
    on the current device goes through the torch expression
    w.flip(2, 3).transpose(0, 1).contiguous(memory_format=
    torch.channels_last), whose values the kernel reproduces bit for
    bit."""
    return _load().mirror_weights_multi(list(weights))


def wgrad_join():
    """The current stream waits for every weight gradient conv2d_split
    has issued on the side stream; a no-op with nothing pending (and
    without the extension loaded, when nothing can be)."""
    if _ext is not None:
        _ext.wgrad_join()


# ------------------------------------------------------ fused max-pool
_POOL_CONFIGS = ((3, 2, 1), (2, 2, 0))  # (k, s, p) compiled in pool.hip


def _pool_int(v):
    if type(v) is int:
        return v
    if isinstance(v, (tuple, list)) and len(v) == 2 and v[0] == v[1] \
            and type(v[0]) is int:
        return v[0]
    return None


def _pool_cfg(kernel_size, stride, padding):
    """(k, s, p) as ints; None entries for non-square / non-int
    arguments (never equal to a compiled configuration)."""
    if stride is None or stride == () or stride == []:
        stride = kernel_size
    return (_pool_int(kernel_size), _pool_int(stride), _pool_int(padding))


def _pool_cfg_supported(x, cfg) -> bool:
    if cfg not in _POOL_CONFIGS or not _nhwc_bf16_ok(x, 8, 2 ** 31):
        return False
    n, _, h, w = x.shape
    k, _, p = cfg
    return n >= 1 and h + 2 * p >= k and w + 2 * p >= k


def fused_pool_enabled() -> bool:
    """KUBESHARE_FUSED_POOL=0 keeps flagged pool modules on the stock
    path (A/B runs, operator escape hatch)."""
    return os.environ.get("KUBESHARE_FUSED_POOL", "1") != "0"


def max_pool_supported(x, kernel_size, stride=None, padding=0) -> bool:
    """True when pool.hip covers the call: (k, s, p) in (3, 2, 1) /
    (2, 2, 0), channels-last bf16 on the GPU, C % 8 == 0, C <= 2048 (one
    256-thread block spans a pixel's channel groups), a non-empty output
    and N*H*W below 2**31 (pixel indices are 32-bit, element offsets
    64-bit)."""
    return _pool_cfg_supported(x, _pool_cfg(kernel_size, stride, padding))


@functools.lru_cache(maxsize=None)
def _max_pool_autograd():
    """Build the autograd.Function once (torch import deferred)."""
    import torch
    from torch.autograd.function import once_differentiable

    class MaxPoolNHWCFn(torch.autograd.Function):
        """NHWC bf16 max-pool via hip/pool.hip. The forward stores a
        one-byte window-local argmax per output element and autograd
        keeps ONLY that (not the pool input); the backward gathers, so
        it needs no memset of dx and no atomics."""

        @staticmethod
        def forward(ctx, x, k, s, p, want_idx):
            out = _load().max_pool_nhwc_fwd(x, k, s, p, want_idx)
            if want_idx:
                ctx.save_for_backward(out[1])
                ctx.input_sizes = list(x.shape)
                ctx.cfg = (k, s, p)
            return out[0]

        @staticmethod
        @once_differentiable
        def backward(ctx, dy):
            (idx,) = ctx.saved_tensors
            dy = _channels_last(dy)
            k, s, p = ctx.cfg
            dx = _load().max_pool_nhwc_bwd(dy, idx, ctx.input_sizes,
                                           k, s, p)
            return dx, None, None, None, None

    return MaxPoolNHWCFn


def max_pool_nhwc(x, kernel_size, stride=None, padding=0):
    """Max-pool through the gfx950 kernels in hip/pool.hip; falls back
    to eager F.max_pool2d for anything max_pool_supported rejects."""
    import torch

    cfg = _pool_cfg(kernel_size, stride, padding)
    if not _pool_cfg_supported(x, cfg):
        return torch.nn.functional.max_pool2d(x, kernel_size, stride,
                                              padding)
    want_idx = torch.is_grad_enabled() and x.requires_grad
    fn = _max_pool_autograd()
    return fn.apply(x, *cfg, want_idx)


# ------------------------------------------- fused BN+ReLU+max-pool
def bn_pool_enabled() -> bool:
    """KUBESHARE_BN_POOL=0 runs BN+ReLU and the max-pool as two ops
    (ops.bn_relu, then ops.max_pool_nhwc) wherever bn_relu_pool would
    have fused them (A/B runs, operator escape hatch)."""
    return os.environ.get("KUBESHARE_BN_POOL", "1") != "0"


def bn_relu_pool_supported(x, kernel_size, stride=None, padding=0) -> bool:
    """True when hip/bn_pool.hip covers BN+ReLU+max-pool of x: what both
    bn_relu and max_pool_supported accept — channels-last bf16 on the
    GPU, C % 8 == 0, 8 <= C <= 2048, (k, s, p) in (3, 2, 1) / (2, 2, 0),
    a non-empty output and N*H*W below 2**31. (The BN output has x's
    shape, so the pool's predicate is evaluated on x itself.)"""
    return _pool_cfg_supported(x, _pool_cfg(kernel_size, stride, padding))


@functools.lru_cache(maxsize=None)
def _bn_relu_pool_autograd():
    """Build the autograd.Function once (torch import deferred)."""
    import torch
    from torch.autograd.function import once_differentiable

    class BNReLUMaxPoolNHWCFn(torch.autograd.Function):
        """max_pool(relu(batch_norm(x))) on NHWC bf16 via hip/bn_pool.hip.
        The full-resolution BN output is never allocated: the forward
        pools while it applies, and autograd keeps x, the one-byte
        window codes and the per-channel vectors; the backward rebuilds
        the pool gradient and the ReLU mask in registers. Values are
        those of ops.max_pool_nhwc(ops.bn_relu(x, bn)), bit for bit in
        forward."""

        @staticmethod
        def forward(ctx, x, weight, bias, running_mean, running_var,
                    training, momentum, eps, k, s, p, want_idx):
            ext = _load()
            w32 = weight.float()
            b32 = bias.float()
            if not training:  # no gradients: bn_relu_pool sees to that
                return ext.bn_relu_pool_fwd_eval(
                    x, w32, b32, running_mean.float(), running_var.float(),
                    eps, k, s, p)[0]
            legacy = bn_reduce_legacy()
            out = ext.bn_relu_pool_fwd_train(
                x, w32, b32, running_mean, running_var, momentum, eps,
                k, s, p, want_idx, legacy)
            if want_idx:
                ctx.save_for_backward(x, out[3], out[1], out[2], w32, b32)
                ctx.cfg = (k, s, p)
                ctx.wdtype = weight.dtype
                ctx.legacy_reduce = legacy
            return out[0]

        @staticmethod
        @once_differentiable
        def backward(ctx, dy):
            x, idx, mean, invstd, w32, b32 = ctx.saved_tensors
            dy = _channels_last(dy)
            dx, dscale, dbias = _load().bn_relu_pool_bwd(
                x, dy, idx, w32, b32, mean, invstd, *ctx.cfg,
                ctx.legacy_reduce)
            return (dx, dscale.to(ctx.wdtype), dbias.to(ctx.wdtype)) + \
                (None,) * 9

    return BNReLUMaxPoolNHWCFn


def bn_relu_pool(x, bn, kernel_size, stride=None, padding=0):
    """max_pool2d(relu(batch_norm(x))) as channels-last bf16 in one
    fused op (hip/bn_pool.hip), using an nn.BatchNorm2d's parameters and
    buffers exactly as bn_relu does; running statistics are updated in
    training mode. Outside bn_relu_pool_supported, in eval mode with
    gradients required, and under KUBESHARE_BN_POOL=0 it runs the
    composition max_pool_nhwc(bn_relu(x, bn), ...), which has its own
    eager fall-backs."""
    import torch

    cfg = _pool_cfg(kernel_size, stride, padding)
    fused = bn_pool_enabled() and _pool_cfg_supported(x, cfg)
    want_idx = False
    if fused:
        want_idx = torch.is_grad_enabled() and (
            x.requires_grad or bn.weight.requires_grad
            or bn.bias.requires_grad)
        fused = bn.training or not want_idx
    if not fused:
        return max_pool_nhwc(bn_relu(x, bn), kernel_size, stride, padding)
    fn = _bn_relu_pool_autograd()
    return fn.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                    bn.training, bn.momentum, bn.eps, *cfg, want_idx)


# --------------------------------------- fused bias+ReLU(+max-pool)
def bias_relu_enabled() -> bool:
    """KUBESHARE_BIAS_RELU=0 routes flagged BN-free models
    (models.vgg.VGGPlain) back to their stock modules (A/B runs,
    operator escape hatch). KUBESHARE_FUSED_POOL=0 keeps its meaning:
    the pools then run the stock module and only bias+ReLU is fused."""
    return os.environ.get("KUBESHARE_BIAS_RELU", "1") != "0"


def bias_relu_supported(x) -> bool:
    """True when hip/bias_relu.hip covers bias+ReLU of x: channels-last
    bf16 on the GPU, C % 8 == 0, 8 <= C <= 2048, not empty and N*H*W
    below 2**31 (bias_relu_pool_supported minus the pool geometry)."""
    if not _nhwc_bf16_ok(x, 8, 2 ** 31):
        return False
    n, _, h, w = x.shape
    return n >= 1 and h >= 1 and w >= 1


def bias_relu_pool_supported(x, kernel_size, stride=None, padding=0) -> bool:
    """True when hip/bias_relu.hip covers bias+ReLU+max-pool of x: what
    bias_relu_supported and max_pool_supported both accept ((k, s, p) in
    (3, 2, 1) / (2, 2, 0) and a non-empty output)."""
    return _pool_cfg_supported(x, _pool_cfg(kernel_size, stride, padding))


@functools.lru_cache(maxsize=None)
def _bias_relu_autograd():
    """Build the autograd.Function once (torch import deferred)."""
    import torch
    from torch.autograd.function import once_differentiable

    class BiasReLUFn(torch.autograd.Function):
        """y = bf16(relu(f32(x) + bias)) on NHWC bf16 via
        hip/bias_relu.hip, out of place. Autograd keeps ONLY y; the
        backward writes dx = (y > 0 ? dy : 0) and sums it into the bias
        gradient in the same pass."""

        @staticmethod
        def forward(ctx, x, bias):
            y = _load().bias_relu_fwd(
                x, bias.detach().float().contiguous())
            ctx.save_for_backward(y)
            ctx.bdtype = bias.dtype
            return y

        @staticmethod
        @once_differentiable
        def backward(ctx, dy):
            (y,) = ctx.saved_tensors
            dy = _channels_last(dy)
            dx, db = _load().bias_relu_bwd(dy, y)
            return dx, db.to(ctx.bdtype)

    return BiasReLUFn


@functools.lru_cache(maxsize=None)
def _bias_relu_pool_autograd():
    """Build the autograd.Function once (torch import deferred)."""
    import torch
    from torch.autograd.function import once_differentiable

    class BiasReLUMaxPoolNHWCFn(torch.autograd.Function):
        """max_pool(relu(x + bias)) on NHWC bf16 via hip/bias_relu.hip.
        The full-resolution activation is never allocated. Autograd
        keeps ONLY the one-byte window codes and the pooled y (the map
        is monotone per channel, so the pooled y is the selected
        element's value and carries its ReLU mask), and nothing at all
        when no gradient is required."""

        @staticmethod
        def forward(ctx, x, bias, k, s, p, want_idx):
            out = _load().bias_relu_pool_fwd(
                x, bias.detach().float().contiguous(), k, s, p, want_idx)
            if want_idx:
                ctx.save_for_backward(out[1], out[0])
                ctx.input_sizes = list(x.shape)
                ctx.cfg = (k, s, p)
                ctx.bdtype = bias.dtype
            return out[0]

        @staticmethod
        @once_differentiable
        def backward(ctx, dy):
            idx, y = ctx.saved_tensors
            dy = _channels_last(dy)
            dx, db = _load().bias_relu_pool_bwd(dy, idx, y, ctx.input_sizes,
                                                *ctx.cfg)
            return dx, db.to(ctx.bdtype), None, None, None, None

    return BiasReLUMaxPoolNHWCFn


def bias_relu(x, bias):
    """relu(x + bias[None, :, None, None]) for a conv output x (N, C, H,
    W) and a per-channel bias (C), in one kernel each way
    (hip/bias_relu.hip) where bias_relu_supported(x) holds:
    y = bf16(relu(f32(x) + f32(bias))). The bias is added in f32 and is
    NOT rounded to bf16 first; that is the one difference from the stock
    autocast modules (a biased conv followed by nn.ReLU), which round
    the bias to bf16 before adding it. Anything else runs the eager
    expression torch.relu(x + bias.to(x.dtype).view(1, -1, 1, 1))."""
    import torch

    if not bias_relu_supported(x) or not bias.is_cuda:
        return torch.relu(x + bias.to(x.dtype).view(1, -1, 1, 1))
    fn = _bias_relu_autograd()
    return fn.apply(x, bias)


def bias_relu_pool(x, bias, kernel_size, stride=None, padding=0):
    """max_pool2d(relu(x + bias)) as one fused op (hip/bias_relu.hip)
    where bias_relu_pool_supported holds; values and gradients are those
    of max_pool_nhwc(bias_relu(x, bias), ...), bit for bit. Outside that
    predicate but inside bias_relu_supported it runs exactly that
    composition; outside both, the eager expression of bias_relu
    followed by F.max_pool2d."""
    import torch

    cfg = _pool_cfg(kernel_size, stride, padding)
    if not _pool_cfg_supported(x, cfg) or not bias.is_cuda:
        if bias_relu_supported(x) and bias.is_cuda:
            return max_pool_nhwc(bias_relu(x, bias), kernel_size, stride,
                                 padding)
        y = torch.relu(x + bias.to(x.dtype).view(1, -1, 1, 1))
        return torch.nn.functional.max_pool2d(y, kernel_size, stride,
                                              padding)
    want_idx = torch.is_grad_enabled() and (x.requires_grad
                                            or bias.requires_grad)
    fn = _bias_relu_pool_autograd()
    return fn.apply(x, bias, *cfg, want_idx)


class PendingBNReLU:
    """A BN+ReLU that has not run yet: the conv output x and its
    nn.BatchNorm2d, handed to the FusedMaxPool2d that follows so that it
    can fuse the three (bn_relu_pool). materialize() runs the BN+ReLU on
    its own. Only fused models create one."""

    __slots__ = ("x", "bn")

    def __init__(self, x, bn):
        self.x = x
        self.bn = bn

    def materialize(self):
        return bn_relu(self.x, self.bn)


def fuse_model(model):
    """Enable the fused BN+ReLU(+add) and max-pool paths on
    kubeshare_amd models (blocks and pool modules check their
    `fused_ops` flag; a flagged ResNet also stages its conv weights,
    see stage_lowp_weights; a flagged VGGPlain runs bias_relu /
    bias_relu_pool after its bias-free convs); verifies the extension
    is importable first (fail-loud on GPU boxes). A ResNet also gets its
    LowpConv2d modules flagged for the forward-convolution data gradient
    (_dgrad_fwd, see dgrad_fwd_flags)."""
    _load()
    for m in model.modules():
        if hasattr(m, "fused_ops"):
            m.fused_ops = True
    from ..models.resnet import ResNet
    if isinstance(model, ResNet):  # VGG: not measured yet (ROADMAP)
        for m, flag in dgrad_fwd_flags(model).items():
            m._dgrad_fwd = flag
    return model
