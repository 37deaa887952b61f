"""Numerics of the NHWC bf16 max-pool kernels (ops/hip/pool.hip) against
F.max_pool2d on the same values in fp32, on the GPU.

Reference layout: the fp32 reference input is made NCHW-contiguous. The
routing rule the kernels implement (start from -inf at the window's
first in-bounds position; `val > maxval || isnan(val)` in row-major scan
order) is the one written out in PyTorch's NCHW pooling kernel, and the
values of max_pool2d do not depend on the memory format, so the layout
of the reference is not part of what is checked here."""
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

CFG_321 = (3, 2, 1)
CFG_220 = (2, 2, 0)
CASES = [
    # 3/2/1: one channel group, odd non-square, last windows hang into
    # the padding
    ((2, 8, 7, 9), CFG_321),
    # C/8 = 3 does not divide the block (idle tail threads)
    ((3, 24, 10, 6), CFG_321),
    ((2, 64, 16, 16), CFG_321),
    ((1, 1536, 5, 5), CFG_321),
    # the predicate's upper bound on C
    ((1, 2048, 4, 4), CFG_321),
    # 2/2/0: last row and column belong to no window -> exactly zero grad
    ((2, 8, 5, 7), CFG_220),
    ((3, 24, 9, 4), CFG_220),
    ((2, 64, 8, 8), CFG_220),
    ((1, 512, 14, 14), CFG_220),
]
KINDS = ["randn", "relu", "const", "negative", "neginf"]


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


def _make(shape, kind, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = torch.randn(shape, device="cuda", generator=g)
    if kind == "relu":          # ~half exact zeros: most windows tie
        r = torch.relu(r)
    elif kind == "const":
        r = torch.full(shape, 0.75, device="cuda")
    elif kind == "negative":    # padding must not win
        r = -r.abs() - 1
    elif kind == "neginf":
        r = torch.full(shape, float("-inf"), device="cuda")
    return _cl(r.to(torch.bfloat16))


def _upstream(y, seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return _cl(torch.randn(y.shape, device="cuda", generator=g)
               .to(torch.bfloat16))


def _reference(x, cfg, dy=None):
    """F.max_pool2d on the same values in fp32 (NCHW, see the module
    docstring); returns (y_ref, dx_ref)."""
    x32 = x.detach().float().contiguous().requires_grad_()
    y_ref = F.max_pool2d(x32, *cfg)
    if dy is None:
        return y_ref.detach(), None
    y_ref.backward(dy.float().contiguous())
    return y_ref.detach(), x32.grad


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,cfg", CASES)
def test_forward_backward_match_fp32_reference(shape, cfg, kind):
    x = _make(shape, kind).requires_grad_()
    assert ops.max_pool_supported(x, *cfg)
    y = ops.max_pool_nhwc(x, *cfg)
    # a silent eager fallback cannot pass
    assert "MaxPoolNHWCFn" in y.grad_fn.name()
    dy = _upstream(y)
    y.backward(dy)
    y_ref, dx_ref = _reference(x, cfg, dy)
    torch.cuda.synchronize()

    assert y.dtype == torch.bfloat16
    assert y.is_contiguous(memory_format=torch.channels_last)
    # the max of bf16 values is exact: no tolerance
    assert torch.equal(y.detach().float(), y_ref)
    dx = x.grad
    assert dx.dtype == torch.bfloat16 and dx.shape == x.shape
    if cfg == CFG_220:
        # each input receives at most one term
        assert torch.equal(dx.float(), dx_ref)
        H, W = shape[2], shape[3]
        if H % 2:
            assert not dx[:, :, H - 1, :].any()
        if W % 2:
            assert not dx[:, :, :, W - 1].any()
    else:
        # one RNE rounding of an f32 sum to bf16 is within 2**-9
        # relative; 2**-7 leaves a factor of four. atol=0 makes every
        # zero of the reference an exact zero, which pins tie routing.
        torch.testing.assert_close(dx.float(), dx_ref, rtol=2 ** -7, atol=0)


@pytest.mark.parametrize("cfg", [CFG_321, CFG_220])
def test_nan_wins_and_routes_like_reference(cfg):
    shape = (1, 8, 6, 6)
    x = _make(shape, "randn", seed=3)
    clean_ref, _ = _reference(x, cfg)
    with torch.no_grad():
        x[0, 5, 3, 2] = float("nan")
    x.requires_grad_()
    y = ops.max_pool_nhwc(x, *cfg)
    assert "MaxPoolNHWCFn" in y.grad_fn.name()
    dy = torch.ones_like(y)
    y.backward(dy)
    y_ref, dx_ref = _reference(x, cfg, dy)
    torch.cuda.synchronize()

    k, s, p = cfg
    OH, OW = y.shape[2], y.shape[3]
    expect_nan = torch.zeros(y.shape, dtype=torch.bool, device="cuda")
    for oh in range(OH):
        for ow in range(OW):
            if oh * s - p <= 3 < oh * s - p + k and \
                    ow * s - p <= 2 < ow * s - p + k:
                expect_nan[0, 5, oh, ow] = True
    assert expect_nan.any()
    yd = y.detach().float()
    assert torch.equal(yd.isnan(), expect_nan)
    assert torch.equal(y_ref.isnan(), expect_nan)
    # the others are unchanged
    assert torch.equal(yd[~expect_nan], clean_ref[~expect_nan])
    assert torch.equal(x.grad.float(), dx_ref)


@pytest.mark.parametrize("cfg", [CFG_321, CFG_220])
def test_expanded_and_nchw_upstream_gradients(cfg):
    shape = (2, 24, 9, 7)
    x = _make(shape, "relu", seed=4).requires_grad_()
    # y.sum().backward(): a stride-0 expanded dy
    y = ops.max_pool_nhwc(x, *cfg)
    y.sum().backward()
    _, dx_ref = _reference(x, cfg, torch.ones_like(y))
    assert torch.equal(x.grad.float(), dx_ref)

    # an NCHW-contiguous dy
    x.grad = None
    y = ops.max_pool_nhwc(x, *cfg)
    dy = _upstream(y).contiguous()
    assert not dy.is_contiguous(memory_format=torch.channels_last)
    y.backward(dy)
    _, dx_ref = _reference(x, cfg, dy)
    if cfg == CFG_220:
        assert torch.equal(x.grad.float(), dx_ref)
    else:
        torch.testing.assert_close(x.grad.float(), dx_ref, rtol=2 ** -7,
                                   atol=0)


@pytest.mark.parametrize("cfg", [CFG_321, CFG_220])
def test_no_grad_forward(cfg):
    x = _make((2, 64, 9, 9), "randn", seed=5).requires_grad_()
    with torch.no_grad():
        y = ops.max_pool_nhwc(x, *cfg)
    assert y.grad_fn is None and not y.requires_grad
    y_ref, _ = _reference(x, cfg)
    assert torch.equal(y.float(), y_ref)
    # an input that needs no gradient takes the same index-free path
    y2 = ops.max_pool_nhwc(x.detach(), *cfg)
    assert y2.grad_fn is None
    assert torch.equal(y2.float(), y_ref)
    # the kernel entry point allocates no index tensor then
    out = ops._load().max_pool_nhwc_fwd(x.detach(), *cfg, False)
    assert len(out) == 1
    out = ops._load().max_pool_nhwc_fwd(x.detach(), *cfg, True)
    assert out[1].dtype == torch.uint8
    assert tuple(out[1].shape) == (2, y.shape[2], y.shape[3], 64)
    assert int(out[1].max()) < cfg[0] * cfg[0]


def _fallback_inputs():
    g = torch.Generator(device="cuda").manual_seed(6)

    def rn(*shape):
        return torch.randn(shape, device="cuda", generator=g)

    return {
        "fp32": (_cl(rn(2, 16, 9, 9)), CFG_321),
        "c12": (_cl(rn(2, 12, 9, 9).to(torch.bfloat16)), CFG_321),
        "nchw": (rn(2, 16, 9, 9).to(torch.bfloat16), CFG_321),
        "k3s1p1": (_cl(rn(2, 16, 9, 9).to(torch.bfloat16)), (3, 1, 1)),
    }


@pytest.mark.parametrize("name", ["fp32", "c12", "nchw", "k3s1p1"])
def test_unsupported_inputs_fall_back_correctly(name):
    x, cfg = _fallback_inputs()[name]
    assert not ops.max_pool_supported(x, *cfg)
    x = x.requires_grad_()
    y = ops.max_pool_nhwc(x, *cfg)
    assert "MaxPoolNHWCFn" not in y.grad_fn.name()
    assert y.dtype == x.dtype
    y_ref, _ = _reference(x, cfg)
    assert torch.equal(y.detach().float(), y_ref)
    y.sum().backward()
    _, dx_ref = _reference(x, cfg, torch.ones_like(y))
    assert torch.equal(x.grad.float(), dx_ref)


def test_forward_is_hipgraph_capturable():
    """One linear branch: warm up on a side stream (as GraphReplayServer
    does), capture, copy new data into the static input, replay."""
    cfg = CFG_321
    static_in = _make((2, 64, 12, 12), "randn", seed=7)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        for _ in range(3):
            ops.max_pool_nhwc(static_in, *cfg)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        static_out = ops.max_pool_nhwc(static_in, *cfg)
    new = _make((2, 64, 12, 12), "negative", seed=8)
    static_in.copy_(new)
    graph.replay()
    torch.cuda.synchronize()
    eager = ops.max_pool_nhwc(new, *cfg)
    assert torch.equal(static_out, eager)
    assert torch.equal(static_out.float(), _reference(new, cfg)[0])


def _run_model(name, shape):
    from kubeshare_amd.models import resnet18, vgg16
    from kubeshare_amd.models.pool import FusedMaxPool2d

    torch.manual_seed(0)
    model = {"resnet18": resnet18, "vgg16": vgg16}[name](num_classes=10)
    model = ops.fuse_model(model).cuda().to(
        memory_format=torch.channels_last)
    pools = [m for m in model.modules() if isinstance(m, FusedMaxPool2d)]
    assert len(pools) == (1 if name == "resnet18" else 5)
    seen = []
    hooks = [m.register_forward_hook(
        lambda mod, inp, out: seen.append(out.grad_fn.name()))
        for m in pools]
    x = _cl(torch.randn(shape, device="cuda"))
    t = torch.randint(0, 10, (shape[0],), device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = F.cross_entropy(model(x), t)
    loss.backward()
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    assert torch.isfinite(loss).item()
    assert all(p.grad is not None and torch.isfinite(p.grad).all()
               for p in model.parameters())
    assert len(seen) == len(pools)
    return seen


@pytest.mark.parametrize("name,shape", [("resnet18", (2, 3, 64, 64)),
                                        ("vgg16", (1, 3, 32, 32))])
def test_fused_models_route_through_the_kernels(name, shape, monkeypatch):
    monkeypatch.delenv("KUBESHARE_FUSED_POOL", raising=False)
    seen = _run_model(name, shape)
    assert all("MaxPoolNHWCFn" in n for n in seen), seen
    monkeypatch.setenv("KUBESHARE_FUSED_POOL", "0")
    seen = _run_model(name, shape)
    assert not any("MaxPoolNHWCFn" in n for n in seen), seen
