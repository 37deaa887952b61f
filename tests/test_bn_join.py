"""ops.bn_join without a GPU: the routing predicate, the environment
switches and the eager fall-back (the composition of two ops.bn_relu
calls, which on the CPU is F.batch_norm + add + relu)."""
import copy
import os
import sys

import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from kubeshare_amd import ops  # noqa: E402


def _bn(C, seed):
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C, generator=g))
        bn.bias.copy_(torch.rand(C, generator=g) - 0.5)
    return bn


def _run(fn, x0, xd0, bn0, bnd0, fork):
    bn, bn_d = copy.deepcopy(bn0), copy.deepcopy(bnd0)
    x = x0.clone().requires_grad_()
    x_d = xd0.clone().requires_grad_()
    out = fn(x, bn, x_d, bn_d, fork)
    y = out[0] if fork else out
    if fork:
        assert out[1] is out[0]  # the eager fall-back returns (y, y)
    g = torch.Generator().manual_seed(5)
    y.backward(torch.randn(y.shape, generator=g).to(y.dtype))
    return [y.detach(), x.grad, x_d.grad, bn.weight.grad, bn.bias.grad,
            bn_d.weight.grad, bn_d.bias.grad, bn.running_mean,
            bn.running_var, bn_d.running_mean, bn_d.running_var]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("fork", [False, True])
def test_cpu_equals_the_composition(dtype, training, fork):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 16, 5, 5, generator=g).to(dtype)
    x_d = torch.randn(2, 16, 5, 5, generator=g).to(dtype)
    bn0, bnd0 = _bn(16, 1).train(training), _bn(16, 2).train(training)
    assert not ops.bn_join_supported(x, x_d)

    def eager(x, bn, x_d, bn_d, fork):
        F = torch.nn.functional
        idn = F.batch_norm(x_d, bn_d.running_mean, bn_d.running_var,
                           bn_d.weight, bn_d.bias, bn_d.training,
                           bn_d.momentum, bn_d.eps)
        y = torch.relu(F.batch_norm(x, bn.running_mean, bn.running_var,
                                    bn.weight, bn.bias, bn.training,
                                    bn.momentum, bn.eps) + idn)
        return (y, y) if fork else y

    got = _run(lambda *a: ops.bn_join(a[0], a[1], a[2], a[3], fork=a[4]),
               x, x_d, bn0, bnd0, fork)
    want = _run(eager, x, x_d, bn0, bnd0, fork)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_env_switches_parse(monkeypatch):
    for name, fn in (("KUBESHARE_BN_JOIN", ops.bn_join_enabled),
                     ("KUBESHARE_BN_MASK", ops.bn_mask_enabled)):
        monkeypatch.delenv(name, raising=False)
        assert fn() is True
        monkeypatch.setenv(name, "0")
        assert fn() is False
        monkeypatch.setenv(name, "1")
        assert fn() is True


def test_supported_predicate_on_cpu_tensors():
    bf = torch.bfloat16
    x = torch.zeros(2, 16, 4, 4, dtype=bf).contiguous(
        memory_format=torch.channels_last)
    assert not ops.bn_join_supported(x, x)            # not on the GPU
    assert not ops.bn_join_supported(x, x[:, :8])     # shapes differ
    assert not ops.bn_join_supported(x[0], x[0])      # not 4-D


def _fused(model):
    """fuse_model's flagging, without its check that the extension is
    built (as in test_bias_relu.py)."""
    for m in model.modules():
        if hasattr(m, "fused_ops"):
            m.fused_ops = True
    return model


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_cpu_models_identical_with_switches_on_and_off(name, monkeypatch):
    from kubeshare_amd import models

    torch.manual_seed(0)
    base = getattr(models, name)(num_classes=10)
    x = torch.randn(2, 3, 32, 32)
    outs = []
    for model, join, mask in ((base, None, None),
                              (_fused(copy.deepcopy(base)), "1", "1"),
                              (_fused(copy.deepcopy(base)), "0", "0")):
        for key, val in (("KUBESHARE_BN_JOIN", join),
                         ("KUBESHARE_BN_MASK", mask)):
            if val is None:
                monkeypatch.delenv(key, raising=False)
            else:
                monkeypatch.setenv(key, val)
        model = copy.deepcopy(model)
        y = model(x)
        y.sum().backward()
        outs.append((y.detach(), model.layer2[0].down[1].weight.grad,
                     model.layer2[0].down[1].running_mean))
    for got in outs[1:]:
        for a, b in zip(got, outs[0]):
            assert torch.equal(a, b)
