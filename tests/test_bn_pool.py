"""CPU-side tests of the fused BN+ReLU+max-pool plumbing: the eager
fall-back of ops.bn_relu_pool, its predicate and switch, the
PendingBNReLU hand-over between a block and the pool module, and the
wiring into the ResNet and VGG models. The kernels are checked on the
GPU in test_bn_pool_gpu.py."""
import os
import sys

import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from kubeshare_amd import ops  # noqa: E402
from kubeshare_amd.models import resnet18, resnet50, vgg16  # noqa: E402
from kubeshare_amd.models.pool import FusedMaxPool2d  # noqa: E402
from kubeshare_amd.models.vgg import ConvBNReLU  # noqa: E402


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


def _bn(C):
    torch.manual_seed(1)
    bn = nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.uniform_(-1.0, 1.0)
        bn.bias.uniform_(-0.5, 0.5)
    return bn


def _eager(x, bn, k, s, p):
    return F.max_pool2d(torch.relu(bn(x)), k, s, p)


@pytest.mark.parametrize("cfg", [(3, 2, 1), (2, 2, 0), (3, 1, 1)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cpu_equals_eager_and_is_unsupported(cfg, dtype):
    import copy
    torch.manual_seed(0)
    x = _cl(torch.randn(2, 16, 9, 11).to(dtype))
    assert not ops.bn_relu_pool_supported(x, *cfg)
    a = _bn(16).to(dtype)
    b = copy.deepcopy(a)
    y = ops.bn_relu_pool(x, a, *cfg)
    assert torch.equal(y, _eager(x, b, *cfg))
    assert torch.equal(a.running_mean, b.running_mean)
    assert torch.equal(a.running_var, b.running_var)


def test_stride_defaults_to_kernel_size():
    x = torch.randn(2, 8, 8, 8)
    bn = _bn(8).eval()
    assert torch.equal(ops.bn_relu_pool(x, bn, 2), _eager(x, bn, 2, 2, 0))


def test_cpu_fallback_is_differentiable():
    import copy
    a = _bn(8)
    b = copy.deepcopy(a)
    x = torch.randn(2, 8, 6, 6).requires_grad_()
    ops.bn_relu_pool(x, a, 3, 2, 1).square().sum().backward()
    x2 = x.detach().clone().requires_grad_()
    _eager(x2, b, 3, 2, 1).square().sum().backward()
    assert torch.equal(x.grad, x2.grad)
    assert torch.equal(a.weight.grad, b.weight.grad)
    assert torch.equal(a.bias.grad, b.bias.grad)


def test_pending_materialize_equals_bn_relu():
    import copy
    x = torch.randn(2, 8, 6, 6)
    a = _bn(8)
    b = copy.deepcopy(a)
    pending = ops.PendingBNReLU(x, a)
    assert pending.x is x and pending.bn is a
    assert torch.equal(pending.materialize(), ops.bn_relu(x, b))
    assert torch.equal(a.running_mean, b.running_mean)


@pytest.mark.parametrize("factory,shape", [(resnet18, (1, 3, 32, 32)),
                                           (vgg16, (1, 3, 32, 32))])
def test_unflagged_models_never_create_a_pending_object(factory, shape,
                                                        monkeypatch):
    made = []

    class Spy(ops.PendingBNReLU):
        def __init__(self, x, bn):
            made.append(bn)
            super().__init__(x, bn)

    monkeypatch.setattr(ops, "PendingBNReLU", Spy)
    model = factory(num_classes=10).eval()
    with torch.no_grad():
        out = model(torch.randn(shape))
    assert out.shape == (shape[0], 10)
    assert made == []


@pytest.mark.parametrize("factory,n", [(resnet18, 1), (vgg16, 5)])
def test_flagged_models_hand_the_bn_to_the_pool(factory, n, monkeypatch):
    """On the CPU every op falls back to eager, so the flagged model must
    agree with the unflagged one; one pending object per pool."""
    made = []

    class Spy(ops.PendingBNReLU):
        def __init__(self, x, bn):
            made.append(bn)
            super().__init__(x, bn)

    monkeypatch.setattr(ops, "PendingBNReLU", Spy)
    monkeypatch.setattr(ops, "_load", lambda: None)
    torch.manual_seed(0)
    model = factory(num_classes=10).eval()
    x = torch.randn(1, 3, 32, 32)
    with torch.no_grad():
        want = model(x)
        ops.fuse_model(model)
        got = model(x)
    assert len(made) == n
    torch.testing.assert_close(got, want)


@pytest.mark.parametrize("env_pool", [None, "0"])
@pytest.mark.parametrize("env_bn_pool", [None, "0"])
def test_flagged_module_with_pending_input_on_cpu_equals_stock(
        monkeypatch, env_pool, env_bn_pool):
    import copy
    for key, val in (("KUBESHARE_FUSED_POOL", env_pool),
                     ("KUBESHARE_BN_POOL", env_bn_pool)):
        if val is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, val)
    a = _bn(16)
    b = copy.deepcopy(a)
    x = _cl(torch.randn(2, 16, 8, 8))
    for m in (FusedMaxPool2d(2, 2), FusedMaxPool2d(3, stride=2, padding=1)):
        want = nn.MaxPool2d(m.kernel_size, m.stride, m.padding)(
            torch.relu(b(x)))
        # unflagged: materialises and pools on the stock path
        assert torch.equal(m(ops.PendingBNReLU(x, a)), want)
        b(x)  # keep the running statistics of the two copies in step
        m.fused_ops = True
        out = m(ops.PendingBNReLU(x, a))
        assert isinstance(out, torch.Tensor)
        assert torch.equal(out, want)
        # a tensor input behaves as before
        assert torch.equal(m(x), F.max_pool2d(x, m.kernel_size, m.stride,
                                              m.padding))


def test_module_routing_by_switch(monkeypatch):
    calls = []
    monkeypatch.setattr(
        ops, "bn_relu_pool",
        lambda x, bn, *a: calls.append(("fused",) + a) or x)
    monkeypatch.setattr(
        ops, "max_pool_nhwc",
        lambda x, *a: calls.append(("pool",) + a) or x)
    monkeypatch.delenv("KUBESHARE_FUSED_POOL", raising=False)
    monkeypatch.delenv("KUBESHARE_BN_POOL", raising=False)
    bn = _bn(8).eval()
    x = torch.randn(1, 8, 6, 6)
    m = FusedMaxPool2d(3, stride=2, padding=1)
    m(ops.PendingBNReLU(x, bn))
    assert calls == []                      # unflagged
    m.fused_ops = True
    m(ops.PendingBNReLU(x, bn))
    assert calls == [("fused", 3, 2, 1)]    # flagged
    monkeypatch.setenv("KUBESHARE_BN_POOL", "0")
    m(ops.PendingBNReLU(x, bn))
    assert calls[1:] == [("pool", 3, 2, 1)]  # two ops
    monkeypatch.setenv("KUBESHARE_FUSED_POOL", "0")
    m(ops.PendingBNReLU(x, bn))
    assert len(calls) == 2                  # stock path
    monkeypatch.delenv("KUBESHARE_FUSED_POOL")
    monkeypatch.delenv("KUBESHARE_BN_POOL")
    m.ceil_mode = True
    m(ops.PendingBNReLU(x, bn))
    assert len(calls) == 2                  # outside the stock conditions


def test_defer_to_pool_marks_the_blocks_in_front_of_a_pool():
    assert ConvBNReLU.defer_to_pool is False
    feats = list(vgg16(num_classes=10).features.children())
    marked = [i for i, m in enumerate(feats)
              if isinstance(m, ConvBNReLU) and m.defer_to_pool]
    assert marked == [1, 4, 8, 12, 16]
    for i in marked:
        assert isinstance(feats[i + 1], FusedMaxPool2d)


def _bn_keys(prefix):
    return [prefix + s for s in ("weight", "bias", "running_mean",
                                 "running_var", "num_batches_tracked")]


def _resnet_keys(block_convs, layers, has_down):
    keys = ["conv1.weight"] + _bn_keys("bn1.")
    for li, n in enumerate(layers, start=1):
        for b in range(n):
            p = f"layer{li}.{b}."
            for c in range(1, block_convs + 1):
                keys += [p + f"conv{c}.weight"] + _bn_keys(p + f"bn{c}.")
            if b == 0 and has_down(li):
                keys += [p + "down.0.weight"] + _bn_keys(p + "down.1.")
    return keys + ["fc.weight", "fc.bias"]


def _vgg_keys():
    keys = []
    for i in (0, 1, 3, 4, 6, 7, 8, 10, 11, 12, 14, 15, 16):
        p = f"features.{i}."
        keys += [p + "conv.weight", p + "conv.bias"] + _bn_keys(p + "bn.")
    for i in (0, 3, 6):
        keys += [f"classifier.{i}.weight", f"classifier.{i}.bias"]
    return keys


@pytest.mark.parametrize("flag", [False, True])
def test_state_dict_keys_unchanged(flag, monkeypatch):
    monkeypatch.setattr(ops, "_load", lambda: None)
    want = {
        "resnet18": _resnet_keys(2, [2, 2, 2, 2], lambda li: li > 1),
        "resnet50": _resnet_keys(3, [3, 4, 6, 3], lambda li: True),
        "vgg16": _vgg_keys(),
    }
    for name, factory in (("resnet18", resnet18), ("resnet50", resnet50),
                          ("vgg16", vgg16)):
        model = factory(num_classes=10)
        if flag:
            ops.fuse_model(model)
        assert list(model.state_dict().keys()) == want[name], name


@pytest.mark.parametrize("env", [None, "0", "1", ""])
def test_env_switch_parsing(monkeypatch, env):
    if env is None:
        monkeypatch.delenv("KUBESHARE_BN_POOL", raising=False)
    else:
        monkeypatch.setenv("KUBESHARE_BN_POOL", env)
    assert ops.bn_pool_enabled() == (env != "0")
    # independent of the pool's own switch
    monkeypatch.setenv("KUBESHARE_FUSED_POOL", "0")
    assert ops.bn_pool_enabled() == (env != "0")
