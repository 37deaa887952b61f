"""ops.bias_relu / ops.bias_relu_pool (ops/hip/bias_relu.hip) and the
fused BN-free VGG16 on the GPU.

Everything is exact except the bias gradient under normal-valued dy:
  forward   torch.relu(x.float() + b.view(1, -1, 1, 1)).to(bf16), f32 b
  pool      y and codes of ext.max_pool_nhwc_fwd(bias_relu(x, b), ...)
  dx        torch.where(y > 0, dy, 0) / the dx of the two-op composition
            ops.max_pool_nhwc(ops.bias_relu(x, b))
  db        integer-valued dy (exact in bf16, every partial sum an
            integer below 2**24): the float64 sum of the oracle's dx,
            exactly, whatever the summation order. Normal dy, small
            shapes: |db - db64| <= n * 2**-24 * sum|dx| per channel with
            n = N*H*W, the first-order bound of any f32 summation order.
The input conditions under which these checks mean something (a mask
exercised both ways, tied windows) are asserted, not assumed."""
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

BF16 = torch.bfloat16
CFG_321 = (3, 2, 1)
CFG_220 = (2, 2, 0)
FN = "BiasReLUFn"
FN_POOL = "BiasReLUMaxPoolNHWCFn"
# Grid formula of the backward kernels (bn_geom_of's stat_blocks, used by
# bias_relu_bwd_kernel and bias_relu_pool_bwd_kernel alike): 512-thread
# blocks of 512/(C/8) rows, at most 1024 of them, grid-stride in groups
# of 4 rows. With C = 8 a block is 512 rows and the stride 1024 * 512 =
# 524,288 rows, so the unrolled body needs N*H*W > 4 * 524,288 =
# 2,097,152 rows. 2049 * 2051 = 4,202,499 rows (67 MB of bf16): two
# passes of the unrolled body, then the remainder loop for the first
# 8,195 lanes. The plain forward kernel has at most 2048 blocks (stride
# 1,048,576): one pass of the unrolled body, then the remainder loop for
# the same 8,195 lanes. Both sizes are odd: the last 3/2/1 windows hang
# into the padding, the last 2/2/0 row and column belong to no window.
# Integer dy in [-2, 2]: |sum| <= 2 * 4,202,499 < 2**24.
BIG = (1, 8, 2049, 2051)
PLAIN_SHAPES = [(2, 8, 7, 9), (3, 24, 10, 6), (2, 64, 16, 16),
                (1, 2048, 4, 4), BIG]
POOL_CASES = [
    ((2, 8, 7, 9), CFG_321),
    ((3, 24, 10, 6), CFG_321),
    ((1, 2048, 4, 4), CFG_321),
    (BIG, CFG_321),
    ((2, 8, 5, 7), CFG_220),
    ((3, 24, 9, 4), CFG_220),
    ((1, 512, 14, 14), CFG_220),
    (BIG, CFG_220),
]
# rand     b ~ U(-0.5, 0.5): about half of y is exactly zero
# allzero  b = -100: everything is zero
KINDS = ["rand", "allzero"]


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


def _input(shape, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return _cl(torch.randn(shape, device="cuda", generator=g).to(BF16))


def _bias(C, kind, seed=10):
    g = torch.Generator(device="cuda").manual_seed(seed)
    b = torch.rand(C, device="cuda", generator=g) - 0.5
    if kind == "allzero":
        b.fill_(-100.0)
    return b


def _int_dy(shape, lim, seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return _cl(torch.randint(-lim, lim + 1, shape, device="cuda",
                             generator=g).to(BF16))


def _normal_dy(shape, seed=2):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return _cl(torch.randn(shape, device="cuda", generator=g).to(BF16))


def _fwd_oracle(x, b):
    return torch.relu(x.float() + b.view(1, -1, 1, 1)).to(BF16)


def _sum64(t):
    return t.double().sum((0, 2, 3))


def _assert_mask_both_ways(y, kind):
    zeros = (y == 0).float().mean().item()
    if kind == "allzero":
        assert zeros == 1.0
    else:
        assert 0.2 <= zeros <= 0.8, zeros


def _assert_db(db, dx_oracle, dy_kind, tag):
    """db (f32, C) against the float64 sum of the oracle's dx."""
    assert db.dtype == torch.float32
    want = _sum64(dx_oracle)
    got = db.double()
    if dy_kind == "int":
        assert torch.equal(got, want), tag
        return
    n = dx_oracle.numel() // dx_oracle.shape[1]
    bound = n * 2.0 ** -24 * _sum64(dx_oracle.abs())
    err = (got - want).abs()
    print({"bias_relu_db": tag, "max_err": err.max().item(),
           "min_slack": (bound - err).min().item()})
    assert (err <= bound).all(), tag


def _run(fn, x0, b0, dy):
    x = x0.detach().clone().requires_grad_()
    b = b0.detach().clone().requires_grad_()
    y = fn(x, b)
    y.backward(dy)
    return y, x.grad, b.grad


# ------------------------------------------------------------- plain op
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", PLAIN_SHAPES)
def test_bias_relu(shape, kind):
    x = _input(shape)
    b = _bias(shape[1], kind)
    assert ops.bias_relu_supported(x)
    big = shape == BIG
    dys = [("int", _int_dy(shape, 2 if big else 8))]
    if not big:
        dys.append(("normal", _normal_dy(shape)))
    want = _fwd_oracle(x, b)
    _assert_mask_both_ways(want, kind)
    for dy_kind, dy in dys:
        y, dx, db = _run(ops.bias_relu, x, b, dy)
        torch.cuda.synchronize()
        assert FN in y.grad_fn.name()  # a silent fall-back cannot pass
        assert y.dtype == BF16 and y.shape == x.shape
        assert y.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(y, want)
        dx_want = torch.where(want > 0, dy, torch.zeros_like(dy))
        assert dx.dtype == BF16
        assert torch.equal(dx, dx_want)
        _assert_db(db, dx_want, dy_kind, (shape, kind, dy_kind))
        if kind == "allzero":
            assert not y.any() and not dx.any()
            assert torch.equal(db, torch.zeros_like(db))
    with torch.no_grad():
        assert torch.equal(ops.bias_relu(x, b), want)


# -------------------------------------------------------------- pool op
def _composition(cfg):
    return lambda x, b: ops.max_pool_nhwc(ops.bias_relu(x, b), *cfg)


def _assert_some_window_ties(y_full, cfg):
    """At least one window whose in-bounds values are all equal (padding
    is -inf for either pool, so it drops out of both)."""
    hi = F.max_pool2d(y_full.float(), *cfg)
    lo = -F.max_pool2d(-y_full.float(), *cfg)
    assert (hi == lo).any()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,cfg", POOL_CASES)
def test_bias_relu_pool(shape, cfg, kind):
    ext = ops._load()
    x = _input(shape)
    b = _bias(shape[1], kind)
    assert ops.bias_relu_pool_supported(x, *cfg)
    big = shape == BIG
    y_full = _fwd_oracle(x, b)
    _assert_mask_both_ways(y_full, kind)
    _assert_some_window_ties(y_full, cfg)
    with torch.no_grad():
        y_full_op = ops.bias_relu(x, b)
    assert torch.equal(y_full_op, y_full)
    y_want, codes_want = ext.max_pool_nhwc_fwd(y_full_op, *cfg, True)

    out = ext.bias_relu_pool_fwd(x, b, *cfg, True)
    assert len(out) == 2
    assert torch.equal(out[0], y_want)
    assert out[1].dtype == torch.uint8
    assert out[1].shape == codes_want.shape
    assert torch.equal(out[1], codes_want)
    out = ext.bias_relu_pool_fwd(x, b, *cfg, False)
    assert len(out) == 1 and torch.equal(out[0], y_want)
    with torch.no_grad():
        y_ng = ops.bias_relu_pool(x, b, *cfg)
    assert y_ng.grad_fn is None and torch.equal(y_ng, y_want)

    dys = [("int", _int_dy(y_want.shape, 2 if big else 8))]
    if not big:
        dys.append(("normal", _normal_dy(y_want.shape)))
    for dy_kind, dy in dys:
        y, dx, db = _run(lambda x, b: ops.bias_relu_pool(x, b, *cfg),
                         x, b, dy)
        yc, dxc, dbc = _run(_composition(cfg), x, b, dy)
        torch.cuda.synchronize()
        assert FN_POOL in y.grad_fn.name()
        assert FN_POOL not in yc.grad_fn.name()
        assert y.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(y, y_want) and torch.equal(yc, y_want)
        assert dx.dtype == BF16 and dx.shape == x.shape
        assert dx.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(dx, dxc)
        _assert_db(db, dxc, dy_kind, (shape, cfg, kind, dy_kind))
        if cfg == CFG_220:
            # odd sizes: the last row / column belongs to no window
            H, W = shape[2], shape[3]
            assert not dx[:, :, H - H % 2:, :].any()
            assert not dx[:, :, :, W - W % 2:].any()
        if kind == "allzero":
            assert not y.any() and not dx.any()
            assert torch.equal(db, torch.zeros_like(db))


# -------------------------------------------------------- autograd state
def test_saved_tensors():
    x = _input((2, 64, 16, 16)).requires_grad_()
    b = _bias(64, "rand").requires_grad_()
    y = ops.bias_relu(x, b)
    saved = y.grad_fn.saved_tensors
    assert len(saved) == 1
    assert saved[0].data_ptr() == y.data_ptr()
    assert saved[0].shape == y.shape and saved[0].dtype == BF16
    assert saved[0].data_ptr() != x.data_ptr()

    for cfg in (CFG_321, CFG_220):
        y = ops.bias_relu_pool(x, b, *cfg)
        saved = y.grad_fn.saved_tensors
        assert len(saved) == 2
        codes, ys = saved
        assert codes.dtype == torch.uint8
        assert tuple(codes.shape) == (2, y.shape[2], y.shape[3], 64)
        assert ys.data_ptr() == y.data_ptr() and ys.shape == y.shape
        assert all(t.data_ptr() != x.data_ptr() for t in saved)
        assert all(t.numel() < x.numel() for t in saved)


def test_db_comes_back_in_the_bias_dtype():
    x = _input((2, 16, 6, 6)).requires_grad_()
    b = _bias(16, "rand").to(BF16).requires_grad_()
    for fn in (ops.bias_relu, lambda x, b: ops.bias_relu_pool(x, b, 2)):
        b.grad = None
        y = fn(x, b)
        assert torch.equal(fn(x.detach(), b.detach()),
                           fn(x.detach(), b.detach().float()))
        y.backward(torch.ones_like(y))
        assert b.grad.dtype == BF16


@pytest.mark.parametrize("cfg", [None, CFG_321, CFG_220])
def test_dy_layouts(cfg):
    shape = (2, 24, 9, 7)
    x0 = _input(shape)
    b0 = _bias(24, "rand")

    def fn(x, b):
        return ops.bias_relu(x, b) if cfg is None else \
            ops.bias_relu_pool(x, b, *cfg)

    with torch.no_grad():
        y0 = fn(x0, b0)
    _, dx1, db1 = _run(fn, x0, b0, torch.ones_like(y0))
    # stride-0 dy
    x = x0.clone().requires_grad_()
    b = b0.clone().requires_grad_()
    fn(x, b).sum().backward()
    assert torch.equal(x.grad, dx1) and torch.equal(b.grad, db1)
    # NCHW-contiguous dy
    dy = _normal_dy(y0.shape)
    _, dx2, db2 = _run(fn, x0, b0, dy)
    dy_nchw = dy.contiguous(memory_format=torch.contiguous_format)
    assert not dy_nchw.is_contiguous(memory_format=torch.channels_last)
    _, dx3, db3 = _run(fn, x0, b0, dy_nchw)
    assert torch.equal(dx3, dx2) and torch.equal(db3, db2)


def test_fallbacks_on_the_gpu():
    g = torch.Generator(device="cuda").manual_seed(5)
    b = _bias(16, "rand")

    def eager(x):
        return torch.relu(x + b.to(x.dtype).view(1, -1, 1, 1))

    x32 = _cl(torch.randn(2, 16, 9, 9, device="cuda", generator=g))
    x12 = _input((2, 12, 9, 9))
    xn = _input((2, 16, 9, 9)).contiguous(
        memory_format=torch.contiguous_format)
    for x, bb in ((x32, b), (x12, _bias(12, "rand")), (xn, b)):
        assert not ops.bias_relu_supported(x)
        want = torch.relu(x + bb.to(x.dtype).view(1, -1, 1, 1))
        assert torch.equal(ops.bias_relu(x, bb), want)
        assert torch.equal(ops.bias_relu_pool(x, bb, 2),
                           F.max_pool2d(want, 2))
    # supported by bias_relu, not by the fused pool: the composition
    x = _input((2, 16, 9, 9)).requires_grad_()
    assert ops.bias_relu_supported(x)
    assert not ops.bias_relu_pool_supported(x, 3, 1, 1)
    y = ops.bias_relu_pool(x, b, 3, 1, 1)
    assert FN_POOL not in y.grad_fn.name()
    assert torch.equal(y, F.max_pool2d(ops.bias_relu(x, b), 3, 1, 1))
    assert torch.equal(ops.bias_relu(x, b), _fwd_oracle(x, b))


# ----------------------------------------------------------------- model
class _Counting:
    """Stands in for the extension module and counts calls by name."""

    def __init__(self, ext):
        self._ext = ext
        self.calls = {}

    def __getattr__(self, name):
        fn = getattr(self._ext, name)

        def wrapped(*a, **k):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a, **k)
        return wrapped


def _model():
    from kubeshare_amd.models import vgg16_plain
    torch.manual_seed(0)
    return ops.fuse_model(vgg16_plain(num_classes=10)).cuda().to(
        memory_format=torch.channels_last)


def _reference_features(model, x):
    """The same bias-free convs, the eager oracle expressions instead of
    the ops."""
    from kubeshare_amd.models.conv import LowpConv2d
    for m in model.features:
        if isinstance(m, LowpConv2d):
            x = m._conv_forward(x, m.weight, None)
            x = _fwd_oracle(x, m.bias.detach())
        elif isinstance(m, torch.nn.MaxPool2d):
            x = F.max_pool2d(x, m.kernel_size, m.stride, m.padding)
    return x


def test_model_features_match_reference_walk(monkeypatch):
    monkeypatch.delenv("KUBESHARE_BIAS_RELU", raising=False)
    monkeypatch.delenv("KUBESHARE_FUSED_POOL", raising=False)
    model = _model().eval()
    x = _cl(torch.randn(2, 3, 32, 32, device="cuda"))
    seen = {}
    h = model.avgpool.register_forward_pre_hook(
        lambda mod, inp: seen.update(features=inp[0].detach()))
    counter = _Counting(ops._load())
    monkeypatch.setattr(ops, "_ext", counter)
    with torch.no_grad(), torch.autocast("cuda", dtype=BF16):
        model(x)
        fused = seen.pop("features")
        assert counter.calls.get("bias_relu_fwd") == 8
        assert counter.calls.get("bias_relu_pool_fwd") == 5
        want = _reference_features(model, x)
        assert fused.dtype == BF16 and fused.shape == (2, 512, 1, 1)
        assert torch.equal(fused, want)
        assert all(c._lowp_weight is None for c in model._lowp_convs)

        # KUBESHARE_FUSED_POOL=0: bias+ReLU fused, stock pools
        counter.calls.clear()
        monkeypatch.setenv("KUBESHARE_FUSED_POOL", "0")
        model(x)
        assert counter.calls.get("bias_relu_fwd") == 13
        assert "bias_relu_pool_fwd" not in counter.calls
        assert "max_pool_nhwc_fwd" not in counter.calls
        assert torch.equal(seen.pop("features"), want)
        monkeypatch.delenv("KUBESHARE_FUSED_POOL")

        # KUBESHARE_BIAS_RELU=0: the stock modules, none of the kernels
        counter.calls.clear()
        monkeypatch.setenv("KUBESHARE_BIAS_RELU", "0")
        model(x)
        assert not any(k.startswith("bias_relu") for k in counter.calls), \
            counter.calls
        stock = seen.pop("features")
        assert stock.shape == want.shape
    h.remove()


def test_model_trains_with_fused_sgd(monkeypatch):
    monkeypatch.delenv("KUBESHARE_BIAS_RELU", raising=False)
    monkeypatch.delenv("KUBESHARE_FUSED_POOL", raising=False)
    model = _model().train()
    opt = ops.FusedSGD(model.parameters(), lr=0.01, momentum=0.9,
                       weight_decay=1e-4)
    x = _cl(torch.randn(2, 3, 32, 32, device="cuda"))
    t = torch.randint(0, 10, (2,), device="cuda")
    counter = _Counting(ops._load())
    monkeypatch.setattr(ops, "_ext", counter)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        with torch.autocast("cuda", dtype=BF16):
            loss = F.cross_entropy(model(x), t)
        loss.backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all()
                   for p in model.parameters())
        opt.step()
        losses.append(loss.item())
    torch.cuda.synchronize()
    assert all(l == l and abs(l) != float("inf") for l in losses), losses
    assert counter.calls.get("bias_relu_bwd") == 3 * 8
    assert counter.calls.get("bias_relu_pool_bwd") == 3 * 5
