"""ops.conv2d_split (ops/hip/conv_split.hip): the stock ATen convolution
with the weight gradient issued on a side stream.

Values: the output and dx are bitwise those of F.conv2d plus autograd on
the same bf16 channels-last inputs (same kernels, same stream order).
MIOpen's tuned weight-gradient solvers accumulate with f32 atomics and
are not run-to-run reproducible, so dW is held to the stock path's own
spread: the stock path runs twice; if its two results agree bitwise the
new op must equal them bitwise, otherwise its largest element-wise
difference to the first stock run must not exceed theirs. Both figures
are printed.

The inputs are small integers. With normal deviates the rule above is a
coin toss on the atomic solvers: every difference is one bf16 rounding
flip of an element whose f32 sum sits on a rounding boundary, and the
largest difference of a pair of runs is the ulp of whichever such
element happened to flip (64->64 3x3 at 14x14, two sessions on MI355X:
stock-stock 0.03125 with split-stock 0.03125, then stock-stock 9.5e-07
with split-stock 0.00195). With integers every product and every partial
sum is exact in f32 whatever the order of the atomics, so the stock path
reproduces itself and the new op is held to the first, bitwise, branch
of the rule. The 64->64 case still prints the stock path's spread on
normal deviates, which tells whether an atomic solver ran.

Lifetimes: autograd frees x and dy as soon as the backward returns,
while the side stream may still read them; the tests then allocate and
poison same-sized tensors on the main stream before they join."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch.nn.functional as F  # noqa: E402

from kubeshare_amd import ops  # noqa: E402
from kubeshare_amd.models.conv import LowpConv2d  # noqa: E402
from kubeshare_amd.utils.tuning import apply_miopen_tuning  # noqa: E402

apply_miopen_tuning()

NEW = "Conv2dSplitFn"
STOCK = "ConvolutionBackward0"
BF16 = torch.bfloat16
CL = torch.channels_last


def _rand(shape, seed, amp=2):
    """Integers in [-amp, amp] (see the module docstring); amp=None gives
    normal deviates."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    if amp is None:
        t = torch.randn(shape, device="cuda", generator=g)
    else:
        t = torch.randint(-amp, amp + 1, shape, device="cuda", generator=g)
    return t.to(BF16).contiguous(memory_format=CL)


def _inputs(n, cin, cout, k, stride, pad, hw, seed=0, amp=2):
    x = _rand((n, cin, hw, hw), seed, amp)
    w = _rand((cout, cin, k, k), seed + 1, amp)
    ho = (hw + 2 * pad - k) // stride + 1
    dy = _rand((n, cout, ho, ho), seed + 2, amp)
    return x, w, dy


def _run(split, x, w, dy, stride, pad, x_grad=True):
    """(y, dx or None, dW) of one forward + backward, synchronized."""
    x = x.detach().clone(memory_format=torch.preserve_format).requires_grad_(
        x_grad)
    w = w.detach().clone(memory_format=torch.preserve_format).requires_grad_()
    if split:
        y = ops.conv2d_split(x, w, stride, pad, 1, 1)
        assert NEW in y.grad_fn.name()
    else:
        y = F.conv2d(x, w, None, stride, pad, 1, 1)
        assert y.grad_fn.name() == STOCK
    y.backward(dy)
    ops.wgrad_join()
    torch.cuda.synchronize()
    assert w.grad.dtype == w.dtype and w.grad.shape == w.shape
    return y.detach(), x.grad, w.grad


def _check_dw(new, s1, s2, tag):
    """The dW rule of the module docstring; returns the stock spread."""
    spread = (s1.float() - s2.float()).abs().max().item()
    diff = (new.float() - s1.float()).abs().max().item()
    print(f"{tag}: dW max |stock - stock| = {spread:g}, "
          f"max |split - stock| = {diff:g}, "
          f"max |stock| = {s1.float().abs().max().item():g}")
    assert new.shape == s1.shape and new.stride() == s1.stride()
    assert torch.isfinite(new).all()
    if torch.equal(s1, s2):
        assert torch.equal(new, s1), tag
    else:
        assert diff <= spread, tag
    return spread


def _kernel_names(fn):
    """Names of the GPU kernels fn() launches (diagnostics only)."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sorted({e.key for e in prof.key_averages()})


CASES = [
    # n, cin, cout, k, stride, pad, hw, x_grad
    pytest.param(2, 8, 16, 3, 1, 1, 9, True, id="3x3-8to16-9x9"),
    pytest.param(2, 16, 32, 1, 2, 0, 8, True, id="1x1s2-16to32-8x8"),
    pytest.param(2, 3, 8, 7, 2, 3, 32, False, id="7x7s2-3to8-32x32-nodx"),
    pytest.param(4, 64, 64, 3, 1, 1, 14, True, id="3x3-64to64-14x14"),
]


@pytest.mark.parametrize("n,cin,cout,k,stride,pad,hw,x_grad", CASES)
def test_values_match_stock(n, cin, cout, k, stride, pad, hw, x_grad):
    x, w, dy = _inputs(n, cin, cout, k, stride, pad, hw)
    _run(False, x, w, dy, stride, pad, x_grad)  # warm-up: solver load
    y1, dx1, dw1 = _run(False, x, w, dy, stride, pad, x_grad)
    y2, dx2, dw2 = _run(False, x, w, dy, stride, pad, x_grad)
    y, dx, dw = _run(True, x, w, dy, stride, pad, x_grad)
    assert torch.equal(y, y1) and torch.equal(y1, y2)
    if x_grad:
        assert dx.stride() == dx1.stride()
        assert torch.equal(dx, dx1) and torch.equal(dx1, dx2)
    else:
        assert dx is None and dx1 is None
    tag = f"{cin}->{cout} {k}x{k} s{stride} @{hw}"
    _check_dw(dw, dw1, dw2, tag)
    if (n, cin, k, hw) == (4, 64, 3, 14):
        # expected to take an atomic split-K solver: on normal deviates
        # two stock runs then differ
        xr, wr, dyr = _inputs(n, cin, cout, k, stride, pad, hw, amp=None)
        r1 = _run(False, xr, wr, dyr, stride, pad)[2]
        r2 = _run(False, xr, wr, dyr, stride, pad)[2]
        spread = (r1.float() - r2.float()).abs().max().item()
        print(f"{tag}: normal deviates, dW max |stock - stock| = {spread:g}")
        if spread == 0:
            def bwd():
                _run(False, xr, wr, dyr, stride, pad)
            print(f"{tag}: stock dW reproducible; kernels:",
                  _kernel_names(bwd))


def test_double_backward_raises():
    x, w, dy = _inputs(2, 8, 16, 3, 1, 1, 9)
    x.requires_grad_()
    w.requires_grad_()
    y = ops.conv2d_split(x, w, 1, 1, 1, 1)
    with pytest.raises(RuntimeError, match="double backward"):
        torch.autograd.grad(y, (x, w), dy, create_graph=True)
    ops.wgrad_join()
    torch.cuda.synchronize()


# ------------------------------------------------- lifetime and ordering
LIFE = dict(n=32, c=64, hw=56)


def _staged_conv(seed):
    torch.manual_seed(seed)
    conv = LowpConv2d(LIFE["c"], LIFE["c"], 3, padding=1, bias=False).cuda().to(
        memory_format=CL)
    with torch.no_grad():  # integer weights: see the module docstring
        conv.weight.copy_(_rand(conv.weight.shape, 100 + seed, 1))
    return conv


def _stage(conv):
    """A bf16 leaf as the staged weight: no CastWeightsFn downstream, so
    nothing joins unless the test does."""
    w = conv.weight.detach().to(BF16).requires_grad_()
    conv._lowp_weight = w
    return w


def _poison(shapes):
    """Eight rounds of same-sized allocations on the current stream,
    filled with NaN: lands in x's, dy's and y's blocks if the allocator
    has handed them back."""
    for _ in range(8):
        junk = [torch.empty(s, device="cuda", dtype=BF16).fill_(float("nan"))
                for s in shapes]
        del junk


def _life_run(monkeypatch, flag, convs, gain=None, opt=None):
    """x -> convs -> (* gain) -> backward(dy) through LowpConv2d with leaf
    staged weights under KUBESHARE_WRW_STREAM=flag; every activation is
    dropped right after backward() and poisoned before the join. Joins
    through opt.step() when given, else through ops.wgrad_join().
    Returns the staged weights' gradients."""
    monkeypatch.setenv("KUBESHARE_WRW_STREAM", flag)
    ext = ops._load()
    shape = (LIFE["n"], LIFE["c"], LIFE["hw"], LIFE["hw"])
    x = _rand(shape, 10, 1).requires_grad_()
    dy = _rand(shape, 11, 1)
    ws = [_stage(c) for c in convs]
    y = x
    for c in convs:
        y = c(y)
        assert (NEW if flag == "1" else STOCK) in y.grad_fn.name()
    if gain is not None:
        y = y * gain.to(BF16).view(1, -1, 1, 1)
    torch.cuda.synchronize()
    assert not ext.wgrad_pending()
    y.backward(dy)
    assert ext.wgrad_pending() == (flag == "1")
    del x, dy, y
    _poison([shape] * 3)
    if opt is not None:
        opt.step()
    else:
        ops.wgrad_join()
    assert not ext.wgrad_pending()
    torch.cuda.synchronize()
    for c in convs:
        c._lowp_weight = None
    return [w.grad for w in ws]


def test_freed_inputs_are_not_reused_before_the_join(monkeypatch):
    conv = _staged_conv(0)
    _life_run(monkeypatch, "0", [conv])  # warm-up
    (s1,) = _life_run(monkeypatch, "0", [conv])
    (s2,) = _life_run(monkeypatch, "0", [conv])
    (new,) = _life_run(monkeypatch, "1", [conv])
    _check_dw(new, s1, s2, "lifetime 64->64 3x3 @56 n32")


def test_join_through_fused_sgd_step(monkeypatch):
    """Two convs and an f32 per-channel gain; only the gain is FusedSGD's,
    and its step() is the only join."""
    convs = [_staged_conv(1), _staged_conv(2)]
    gain = torch.nn.Parameter(torch.ones(LIFE["c"], device="cuda"))
    opt = ops.FusedSGD([gain], lr=0.01, momentum=0.9, graph_mode="off")

    def run(flag):
        opt.zero_grad()
        with torch.no_grad():  # every run starts from the same state
            gain.fill_(1.0)
            opt.momenta[0].zero_()
        return _life_run(monkeypatch, flag, convs, gain, opt)

    run("0")  # warm-up
    s1, s2, new = run("0"), run("0"), run("1")
    for i in range(2):
        _check_dw(new[i], s1[i], s2[i], f"FusedSGD join, conv {i}")
    assert torch.isfinite(gain).all()


# ---------------------------------------------------------------- routing
def _graph_names(root):
    seen, stack = set(), [root]
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        stack.extend(n for n, _ in fn.next_functions)
    return [fn.name() for fn in seen]


def test_routing_of_one_conv(monkeypatch):
    monkeypatch.delenv("KUBESHARE_WRW_STREAM", raising=False)
    conv = LowpConv2d(8, 16, 3, padding=1, bias=False).cuda().to(
        memory_format=CL)
    x16 = _rand((2, 8, 9, 9), 0)
    w16 = conv.weight.detach().to(BF16).requires_grad_()
    # the staged bf16 path
    conv._lowp_weight = w16
    assert NEW in conv(x16).grad_fn.name()
    # an f32 input under bf16 autocast is cast as autocast casts it
    with torch.autocast("cuda", dtype=BF16):
        y = conv(x16.float())
    assert NEW in y.grad_fn.name() and y.dtype == BF16
    assert torch.equal(y, conv(x16))
    # the switch
    monkeypatch.setenv("KUBESHARE_WRW_STREAM", "0")
    assert conv(x16).grad_fn.name() == STOCK
    monkeypatch.delenv("KUBESHARE_WRW_STREAM")
    # fp32: a staged f32 weight, and nothing staged at all
    conv._lowp_weight = conv.weight.detach().clone().requires_grad_()
    assert conv(x16.float()).grad_fn.name() == STOCK
    conv._lowp_weight = None
    assert conv(x16.float()).grad_fn.name() == STOCK
    # bias
    biased = LowpConv2d(8, 16, 3, padding=1, bias=True).cuda().to(BF16)
    biased._lowp_weight = w16
    assert biased(x16).grad_fn.name() == STOCK
    # CPU
    cpu = LowpConv2d(8, 16, 3, padding=1, bias=False)
    cpu._lowp_weight = cpu.weight.detach().clone().requires_grad_()
    assert cpu(torch.randn(2, 8, 9, 9)).grad_fn.name() == STOCK


def _small_resnet50():
    from kubeshare_amd.models import resnet50
    torch.manual_seed(0)
    model = ops.fuse_model(resnet50(num_classes=10)).cuda().to(
        memory_format=CL)
    x = torch.randn(2, 3, 32, 32, device="cuda").contiguous(memory_format=CL)
    target = torch.tensor([1, 7], device="cuda")
    return model, x, target


def _forward(model, x, target):
    with torch.autocast("cuda", dtype=BF16):
        return F.cross_entropy(model(x), target)


def test_resnet50_routes_all_53_convs_and_trains(monkeypatch):
    monkeypatch.delenv("KUBESHARE_WRW_STREAM", raising=False)
    monkeypatch.delenv("KUBESHARE_LOWP_WEIGHTS", raising=False)
    model, x, target = _small_resnet50()
    opt = ops.FusedSGD(model.parameters(), lr=0.01, momentum=0.9,
                       weight_decay=1e-4)
    loss = _forward(model, x, target)
    names = _graph_names(loss.grad_fn)
    assert sum(NEW in n for n in names) == 53
    assert not any(n == STOCK for n in names)
    loss.backward()
    opt.step()
    assert not ops._load().wgrad_pending()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()
    for p in model.parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32
        assert p.grad.stride() == p.stride()
        assert torch.isfinite(p.grad).all() and torch.isfinite(p).all()
    loss2 = _forward(model, x, target)
    torch.cuda.synchronize()
    assert torch.isfinite(loss2).all()


@pytest.mark.parametrize("var", ["KUBESHARE_WRW_STREAM",
                                 "KUBESHARE_LOWP_WEIGHTS"])
def test_resnet50_switches_give_the_stock_node(monkeypatch, var):
    monkeypatch.delenv("KUBESHARE_WRW_STREAM", raising=False)
    monkeypatch.delenv("KUBESHARE_LOWP_WEIGHTS", raising=False)
    monkeypatch.setenv(var, "0")
    model, x, target = _small_resnet50()
    names = _graph_names(_forward(model, x, target).grad_fn)
    assert not any(NEW in n for n in names)
    assert sum(n == STOCK for n in names) == 53


# ---------------------------------------------------------------- capture
def test_capture_does_not_fork_and_replays_equal():
    ext = ops._load()
    x, w, dy = _inputs(2, 8, 16, 3, 1, 1, 9, seed=20)
    xs = x.clone(memory_format=torch.preserve_format).requires_grad_()
    wl = w.clone(memory_format=torch.preserve_format).requires_grad_()

    def fwd_bwd():
        y = ops.conv2d_split(xs, wl, 1, 1, 1, 1)
        dx, dw = torch.autograd.grad(y, (xs, wl), dy)
        return y, dx, dw

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fwd_bwd()  # warm-up off the default stream; this one forks
        ops.wgrad_join()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert not ext.wgrad_pending()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y, dx, dw = fwd_bwd()
    assert not ext.wgrad_pending()  # both halves went into the capture
    # replay on new values, against eager stock runs on the same values
    x2, w2, dy2 = _inputs(2, 8, 16, 3, 1, 1, 9, seed=30)
    with torch.no_grad():
        xs.copy_(x2)
        wl.copy_(w2)
        dy.copy_(dy2)
    graph.replay()
    torch.cuda.synchronize()
    y1, dx1, dw1 = _run(False, x2, w2, dy2, 1, 1)
    _, _, dw2_ = _run(False, x2, w2, dy2, 1, 1)
    assert torch.equal(y, y1) and torch.equal(dx, dx1)
    _check_dw(dw, dw1, dw2_, "graph replay")
