"""CPU-side tests of the fused max-pool plumbing: eager fallback of
ops.max_pool_nhwc, the support predicate, the FusedMaxPool2d module and
its wiring into the ResNet and VGG models. The kernels themselves are
checked on the GPU in test_pool_gpu.py."""
import os
import sys

import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from kubeshare_amd import ops  # noqa: E402
from kubeshare_amd.models import resnet50, vgg16  # noqa: E402
from kubeshare_amd.models.pool import FusedMaxPool2d  # noqa: E402


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


# (input, (k, s, p)): the two kernel configurations in bf16
# channels-last, an unsupported configuration, and an fp32 input
def _cpu_cases():
    torch.manual_seed(0)
    bf = _cl(torch.randn(2, 16, 9, 11).to(torch.bfloat16))
    return [
        (bf, (3, 2, 1)),
        (bf, (2, 2, 0)),
        (bf, (3, 1, 1)),
        (_cl(torch.randn(2, 16, 9, 11)), (3, 2, 1)),
    ]


@pytest.mark.parametrize("case", range(4))
def test_cpu_matches_eager_and_is_unsupported(case):
    x, (k, s, p) = _cpu_cases()[case]
    assert not ops.max_pool_supported(x, k, s, p)
    y = ops.max_pool_nhwc(x, k, s, p)
    assert torch.equal(y, F.max_pool2d(x, k, s, p))


def test_stride_defaults_to_kernel_size():
    x = _cpu_cases()[0][0]
    assert torch.equal(ops.max_pool_nhwc(x, 2), F.max_pool2d(x, 2))


def test_cpu_fallback_is_differentiable():
    x = torch.randn(1, 8, 6, 6).requires_grad_()
    ops.max_pool_nhwc(x, 2, 2, 0).sum().backward()
    x2 = x.detach().clone().requires_grad_()
    F.max_pool2d(x2, 2, 2, 0).sum().backward()
    assert torch.equal(x.grad, x2.grad)


def test_module_is_a_maxpool_and_equals_stock_unflagged():
    m = FusedMaxPool2d(3, stride=2, padding=1)
    assert isinstance(m, nn.MaxPool2d)
    assert FusedMaxPool2d.fused_ops is False and m.fused_ops is False
    assert not list(m.parameters()) and not list(m.buffers())
    x = torch.randn(2, 16, 9, 11)
    assert torch.equal(m(x), nn.MaxPool2d(3, stride=2, padding=1)(x))


def test_models_use_it_without_new_state_dict_keys():
    r, v = resnet50(num_classes=10), vgg16(num_classes=10)
    assert isinstance(r.maxpool, FusedMaxPool2d)
    assert (r.maxpool.kernel_size, r.maxpool.stride,
            r.maxpool.padding) == (3, 2, 1)
    for model in (r, v):
        for key in model.state_dict():
            assert "pool" not in key, key
    # the pools sit between parameterised layers: numbering unchanged
    assert not any(k.startswith(("features.2.", "features.5."))
                   for k in v.state_dict())
    assert any(k.startswith("features.3.") for k in v.state_dict())


def test_vgg_layer_positions_do_not_move():
    feats = list(vgg16(num_classes=10).features.children())
    assert len(feats) == 18
    pools = [i for i, m in enumerate(feats) if isinstance(m, nn.MaxPool2d)]
    assert pools == [2, 5, 9, 13, 17]
    for i in pools:
        assert isinstance(feats[i], FusedMaxPool2d)
        assert (feats[i].kernel_size, feats[i].stride,
                feats[i].padding) == (2, 2, 0)


def test_small_models_stay_on_stock_pool():
    from kubeshare_amd.models.small import mnist_cnn
    assert not any(isinstance(m, FusedMaxPool2d)
                   for m in mnist_cnn(10).modules())


def test_fuse_model_flags_the_pools(monkeypatch):
    monkeypatch.setattr(ops, "_load", lambda: None)
    r = ops.fuse_model(resnet50(num_classes=10))
    assert r.maxpool.fused_ops is True
    v = ops.fuse_model(vgg16(num_classes=10))
    pools = [m for m in v.modules() if isinstance(m, FusedMaxPool2d)]
    assert len(pools) == 5 and all(m.fused_ops for m in pools)
    # a fresh module is untouched (the flag is set per instance)
    assert FusedMaxPool2d(2, 2).fused_ops is False


@pytest.mark.parametrize("env", [None, "0", "1"])
def test_flagged_module_on_cpu_equals_stock(monkeypatch, env):
    if env is None:
        monkeypatch.delenv("KUBESHARE_FUSED_POOL", raising=False)
    else:
        monkeypatch.setenv("KUBESHARE_FUSED_POOL", env)
    assert ops.fused_pool_enabled() == (env != "0")
    m = FusedMaxPool2d(2, 2)
    m.fused_ops = True
    x = _cl(torch.randn(2, 16, 8, 8).to(torch.bfloat16))
    assert torch.equal(m(x), F.max_pool2d(x, 2, 2))


def test_env_switch_bypasses_the_op(monkeypatch):
    calls = []
    monkeypatch.setattr(ops, "max_pool_nhwc",
                        lambda x, *a, **kw: calls.append(a) or
                        F.max_pool2d(x, *a, **kw))
    m = FusedMaxPool2d(3, stride=2, padding=1)
    x = torch.randn(1, 8, 6, 6)
    m(x)
    assert calls == []            # unflagged
    m.fused_ops = True
    monkeypatch.setenv("KUBESHARE_FUSED_POOL", "0")
    m(x)
    assert calls == []            # flagged, switched off
    monkeypatch.delenv("KUBESHARE_FUSED_POOL")
    m(x)
    assert calls == [(3, 2, 1)]   # flagged
