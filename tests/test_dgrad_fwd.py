"""Stride-1 data gradients as forward convolutions on mirrored weights:
the identity itself and the model-side routing rule, on the CPU.

dx of y = conv(x, W) with stride 1 is conv(dy, Wm, padding=R-1-p) with
Wm[c,k,r,s] = W[k,c,R-1-r,S-1-s]. On small integers every product and
sum is exact in f32, so the two sides are compared with torch.equal."""
import os
import sys

import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch.nn.functional as F  # noqa: E402

from kubeshare_amd import ops  # noqa: E402
from kubeshare_amd.models import resnet50  # noqa: E402
from kubeshare_amd.models.conv import LowpConv2d  # noqa: E402


def _mirror(w):
    return w.flip(2, 3).transpose(0, 1).contiguous(
        memory_format=torch.channels_last)


@pytest.mark.parametrize("cin,cout,k,h,w", [
    pytest.param(16, 32, 1, 6, 5, id="1x1-16to32-6x5"),
    pytest.param(16, 16, 3, 5, 7, id="3x3-16to16-5x7"),
    pytest.param(8, 24, 3, 4, 4, id="3x3-8to24-4x4"),
])
def test_identity_on_integers(cin, cout, k, h, w):
    g = torch.Generator().manual_seed(k * 100 + cin)
    x = torch.randint(-2, 3, (2, cin, h, w), generator=g).float()
    wt = torch.randint(-2, 3, (cout, cin, k, k), generator=g).float()
    dy = torch.randint(-2, 3, (2, cout, h, w), generator=g).float()
    p = k // 2
    x.requires_grad_()
    F.conv2d(x, wt, None, 1, p).backward(dy)
    wm = _mirror(wt)
    assert wm.shape == (cin, cout, k, k)
    dx = F.conv2d(dy, wm, None, 1, k - 1 - p)
    assert torch.equal(dx, x.grad)


def _flagged(model):
    return {name for name, m in model.named_modules()
            if isinstance(m, LowpConv2d) and m._dgrad_fwd}


def _fused_resnet50(monkeypatch):
    # the flags need no extension: keep the test GPU- and build-free
    monkeypatch.setattr(ops, "_load", lambda: None)
    return ops.fuse_model(resnet50(num_classes=10))


UNCOVERED = {"layer2.0.conv1", "layer3.0.conv1", "layer4.0.conv1"}


def test_resnet50_flags_the_43_convs(monkeypatch):
    monkeypatch.delenv("KUBESHARE_DGRAD_FWD", raising=False)
    model = _fused_resnet50(monkeypatch)
    flagged = _flagged(model)
    assert len(flagged) == 43
    assert not flagged & UNCOVERED
    assert "conv1" not in flagged  # the stem
    mods = dict(model.named_modules())
    for name in flagged:
        m = mods[name]
        assert m.stride == (1, 1) and m.groups == 1 and m.bias is None
        assert m.kernel_size in ((1, 1), (3, 3))
    stride2 = {n for n, m in mods.items()
               if isinstance(m, LowpConv2d) and m.stride != (1, 1)}
    assert len(stride2) == 7 and not flagged & stride2
    # the table of the 13 mirrored shapes: 30 1x1 convs and 13 3x3 convs
    assert sum(mods[n].kernel_size == (1, 1) for n in flagged) == 30
    assert sum(mods[n].kernel_size == (3, 3) for n in flagged) == 13


def test_switch_values(monkeypatch):
    monkeypatch.setenv("KUBESHARE_DGRAD_FWD", "0")
    assert _flagged(_fused_resnet50(monkeypatch)) == set()
    monkeypatch.delenv("KUBESHARE_DGRAD_FWD")
    default = _flagged(_fused_resnet50(monkeypatch))
    for mode, k in (("1x1", (1, 1)), ("3x3", (3, 3))):
        monkeypatch.setenv("KUBESHARE_DGRAD_FWD", mode)
        model = _fused_resnet50(monkeypatch)
        mods = dict(model.named_modules())
        want = {n for n in default if mods[n].kernel_size == k}
        assert _flagged(model) == want and want
    monkeypatch.setenv("KUBESHARE_DGRAD_FWD", "all")
    every = _flagged(_fused_resnet50(monkeypatch))
    assert every == default | UNCOVERED
    monkeypatch.setenv("KUBESHARE_DGRAD_FWD", "yes")
    with pytest.raises(ValueError, match="KUBESHARE_DGRAD_FWD"):
        _fused_resnet50(monkeypatch)


def test_unflagged_model_and_cpu_conv_get_no_mirror(monkeypatch):
    monkeypatch.delenv("KUBESHARE_DGRAD_FWD", raising=False)
    # a plain (unfused) model carries no flag at all
    assert _flagged(resnet50(num_classes=10)) == set()
    # a CPU model stages nothing, so no conv ever holds a mirror, flagged
    # or not; its forward and backward are the stock ones
    model = _fused_resnet50(monkeypatch)
    convs = model._lowp_convs
    assert ops.stage_lowp_weights(convs) == []
    assert all(m._lowp_mirror is None and m._lowp_weight is None
               for m in convs)
    conv = LowpConv2d(8, 8, 3, padding=1, bias=False)
    conv._dgrad_fwd = True
    x = torch.randn(2, 8, 5, 5, requires_grad=True)
    y = conv(x)
    assert conv._lowp_mirror is None
    assert y.grad_fn.name() == "ConvolutionBackward0"
    ops.clear_lowp_weights([conv])
    assert conv._lowp_mirror is None


def test_deterministic_attribute_keeps_the_default_off(monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.delenv("KUBESHARE_DGRAD_FWD", raising=False)
    assert not ops.dgrad_fwd_active()
    for mode, want in (("0", False), ("1x1", True), ("3x3", True),
                       ("all", True)):
        monkeypatch.setenv("KUBESHARE_DGRAD_FWD", mode)
        assert ops.dgrad_fwd_active() == want
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", False)
    monkeypatch.delenv("KUBESHARE_DGRAD_FWD")
    assert ops.dgrad_fwd_active()
    monkeypatch.setenv("KUBESHARE_DGRAD_FWD", "0")
    assert not ops.dgrad_fwd_active()
