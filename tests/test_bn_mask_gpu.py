"""The ReLU mask as bits (KUBESHARE_BN_MASK) on the GPU.

A residual BN in training mode saves one byte per 8 channels (bit j set
iff the stored bf16 y of channel j is > 0) instead of y; its backward
stats kernel reads that byte where it read y. The predicate is the same,
so everything is asserted with torch.equal against KUBESHARE_BN_MASK=0,
which keeps the y-reading kernels."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from kubeshare_amd import ops  # noqa: E402

# the first four shapes of test_bn_join_gpu.py
SHAPES = [(2, 8, 3, 3), (2, 24, 5, 5), (3, 2048, 7, 7), (17, 256, 64, 64)]
# two gradients / fork with one consumer / unforked
MODES = ["fork2", "fork1", "plain"]


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


def _rand(shape, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return _cl(torch.randn(shape, device="cuda", generator=g)
               .to(torch.bfloat16))


def _bn(C, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    bn = torch.nn.BatchNorm2d(C).cuda()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C, device="cuda", generator=g))
        bn.weight[::3] = 0.0
        bn.bias.copy_(torch.rand(C, device="cuda", generator=g) - 0.5)
    return bn


def _backward(out, mode, g1, g2):
    if mode == "plain":
        out.backward(g1)
        return out
    y, y2 = out
    if mode == "fork2":
        torch.autograd.backward([y, y2], [g1, g2])
    else:
        y2.backward(g2)
    return y


def _residual(shape, mode, monkeypatch, mask, x=None):
    """bn_relu with res under KUBESHARE_BN_MASK=mask."""
    monkeypatch.setenv("KUBESHARE_BN_MASK", mask)
    assert ops.bn_mask_enabled() == (mask == "1")
    x = (_rand(shape, 0) if x is None else x).clone().requires_grad_()
    res = _rand(shape, 1).requires_grad_()
    bn = _bn(shape[1], 10)
    out = ops.bn_relu(x, bn, res=res, fork=mode != "plain")
    y0 = out if mode == "plain" else out[0]
    saved = y0.grad_fn.saved_tensors
    y = _backward(out, mode, _rand(shape, 2), _rand(shape, 3))
    torch.cuda.synchronize()
    return {"y": y.detach(), "dx": x.grad, "dres": res.grad,
            "dscale": bn.weight.grad, "dbias": bn.bias.grad,
            "rm": bn.running_mean, "rv": bn.running_var}, saved


def _assert_saved(saved, y, shape, masked):
    N, C, H, W = shape
    held_y = any(t.data_ptr() == y.data_ptr() for t in saved)
    masks = [t for t in saved if t.dtype == torch.uint8]
    if masked:
        assert not held_y
        assert len(masks) == 1
        assert tuple(masks[0].shape) == (N, H, W, C // 8)
        # bit j of a byte <=> the stored y of channel 8*cg + j is > 0
        want = (y.permute(0, 2, 3, 1).reshape(N, H, W, C // 8, 8) > 0)
        weights = 2 ** torch.arange(8, device="cuda")
        assert torch.equal(masks[0].long(), (want.long() * weights).sum(-1))
    else:
        assert held_y and not masks


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_residual_bn_mask_on_off(shape, mode, monkeypatch):
    on, saved_on = _residual(shape, mode, monkeypatch, "1")
    off, saved_off = _residual(shape, mode, monkeypatch, "0")
    _assert_saved(saved_on, on["y"], shape, True)
    _assert_saved(saved_off, off["y"], shape, False)
    for key in on:
        assert torch.equal(on[key], off[key]), key


def test_nan(monkeypatch):
    shape = (2, 16, 5, 5)
    x = _rand(shape, 0)
    with torch.no_grad():
        x[1, 5, 3, 2] = float("nan")
    on, _ = _residual(shape, "fork2", monkeypatch, "1", x=x)
    off, _ = _residual(shape, "fork2", monkeypatch, "0", x=x)
    assert off["y"].isnan().any() and not off["y"].isnan().all()
    assert off["dx"].isnan().any()
    for key in ("y", "dx", "dres"):
        a, b = on[key], off[key]
        assert torch.equal(a.isnan(), b.isnan()), key
        assert torch.equal(a[~a.isnan()], b[~b.isnan()]), key


def test_non_residual_and_eval_keep_their_saved_tensors(monkeypatch):
    """Only training-mode residual BNs with ReLU have a mask."""
    monkeypatch.setenv("KUBESHARE_BN_MASK", "1")
    shape = (2, 24, 5, 5)
    x = _rand(shape, 0).requires_grad_()
    bn = _bn(24, 10)
    y = ops.bn_relu(x, bn)
    assert not any(t.dtype == torch.uint8 for t in y.grad_fn.saved_tensors)
    bn.eval()
    y = ops.bn_relu(x, bn, res=_rand(shape, 1))
    assert not any(t.dtype == torch.uint8 for t in y.grad_fn.saved_tensors)
    y.backward(_rand(shape, 2))
    assert torch.isfinite(x.grad.float()).all()


def _join(shape, mode, monkeypatch, mask):
    monkeypatch.setenv("KUBESHARE_BN_MASK", mask)
    monkeypatch.delenv("KUBESHARE_BN_JOIN", raising=False)
    x = _rand(shape, 0).requires_grad_()
    x_d = _rand(shape, 1).requires_grad_()
    bn, bn_d = _bn(shape[1], 10), _bn(shape[1], 11)
    out = ops.bn_join(x, bn, x_d, bn_d, fork=mode != "plain")
    y0 = out if mode == "plain" else out[0]
    assert "BNJoinFn" in y0.grad_fn.name()
    saved = y0.grad_fn.saved_tensors
    y = _backward(out, mode, _rand(shape, 2), _rand(shape, 3))
    torch.cuda.synchronize()
    return {"y": y.detach(), "dx": x.grad, "dx_d": x_d.grad,
            "dscale": bn.weight.grad, "dbias": bn.bias.grad,
            "dscale_d": bn_d.weight.grad, "dbias_d": bn_d.bias.grad}, saved


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_join_mask_on_off(shape, mode, monkeypatch):
    on, saved_on = _join(shape, mode, monkeypatch, "1")
    off, saved_off = _join(shape, mode, monkeypatch, "0")
    _assert_saved(saved_on, on["y"], shape, True)
    _assert_saved(saved_off, off["y"], shape, False)
    for key in on:
        assert torch.equal(on[key], off[key]), key
