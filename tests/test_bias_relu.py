"""ops.bias_relu / ops.bias_relu_pool and the BN-free VGG16
(models.vgg16_plain) without a GPU: the eager fall-backs, the predicates,
the model's layout and the bench_worker parser."""
import os
import sys

import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch.nn.functional as F  # noqa: E402

from kubeshare_amd import ops  # noqa: E402
from kubeshare_amd.models import build_model, vgg16_plain  # noqa: E402

CFGS = [(3, 2, 1), (2, 2, 0), (3, 1, 1)]  # the last one is not compiled
CONV_IDX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
POOL_IDX = (4, 9, 16, 23, 30)


def _eager(x, b):
    return torch.relu(x + b.to(x.dtype).view(1, -1, 1, 1))


def _inputs(dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 16, 9, 11, generator=g).to(dtype)
    b = torch.rand(16, generator=g) - 0.5
    return x, b


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bias_relu_cpu_equals_eager(dtype):
    x, b = _inputs(dtype)
    y = ops.bias_relu(x, b)
    assert y.dtype == dtype
    assert torch.equal(y, _eager(x, b))


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bias_relu_pool_cpu_equals_eager(dtype, cfg):
    x, b = _inputs(dtype)
    y = ops.bias_relu_pool(x, b, *cfg)
    assert y.dtype == dtype
    assert torch.equal(y, F.max_pool2d(_eager(x, b), *cfg))


@pytest.mark.parametrize("cfg", [None] + CFGS)
def test_cpu_gradients_equal_eager(cfg):
    x0, b0 = _inputs(torch.float32, seed=1)
    grads = []
    for fused in (True, False):
        x = x0.clone().requires_grad_()
        b = b0.clone().requires_grad_()
        if cfg is None:
            y = ops.bias_relu(x, b) if fused else _eager(x, b)
        elif fused:
            y = ops.bias_relu_pool(x, b, *cfg)
        else:
            y = F.max_pool2d(_eager(x, b), *cfg)
        g = torch.Generator().manual_seed(2)
        y.backward(torch.randn(y.shape, generator=g))
        grads.append((x.grad, b.grad))
    assert grads[0][0] is not None and grads[0][1] is not None
    assert torch.equal(grads[0][0], grads[1][0])
    assert torch.equal(grads[0][1], grads[1][1])


def test_predicates_false_on_cpu():
    x = torch.randn(2, 16, 8, 8).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    assert not ops.bias_relu_supported(x)
    for cfg in CFGS:
        assert not ops.bias_relu_pool_supported(x, *cfg)
    assert not ops.bias_relu_supported(x[0])


def test_stride_defaults_to_kernel_size():
    x, b = _inputs(torch.float32)
    assert torch.equal(ops.bias_relu_pool(x, b, 2),
                       ops.bias_relu_pool(x, b, 2, 2, 0))
    assert torch.equal(ops.bias_relu_pool(x, b, 2),
                       F.max_pool2d(_eager(x, b), 2))
    assert ops.bias_relu_pool(x, b, 2).shape == (2, 16, 4, 5)


def test_switch(monkeypatch):
    monkeypatch.delenv("KUBESHARE_BIAS_RELU", raising=False)
    assert ops.bias_relu_enabled()
    monkeypatch.setenv("KUBESHARE_BIAS_RELU", "0")
    assert not ops.bias_relu_enabled()


def test_vgg16_plain_state_dict_is_torchvisions():
    chans = [3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512,
             512]
    want = {}
    for n, i in enumerate(CONV_IDX):
        want[f"features.{i}.weight"] = (chans[n + 1], chans[n], 3, 3)
        want[f"features.{i}.bias"] = (chans[n + 1],)
    for i, (o, k) in zip((0, 3, 6), ((4096, 25088), (4096, 4096),
                                     (1000, 4096))):
        want[f"classifier.{i}.weight"] = (o, k)
        want[f"classifier.{i}.bias"] = (o,)
    sd = vgg16_plain().state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == want


def test_vgg16_plain_layout():
    from kubeshare_amd.models.conv import LowpConv2d
    from kubeshare_amd.models.pool import FusedMaxPool2d

    m = vgg16_plain(num_classes=10)
    assert len(m.features) == 31
    for i, mod in enumerate(m.features):
        if i in CONV_IDX:
            assert isinstance(mod, LowpConv2d) and mod.bias is not None
            assert mod.kernel_size == (3, 3) and mod.padding == (1, 1)
        elif i in POOL_IDX:
            assert isinstance(mod, FusedMaxPool2d)
            assert mod.kernel_size == 2 and mod.stride == 2
        else:
            assert isinstance(mod, torch.nn.ReLU) and mod.inplace
    assert isinstance(m.avgpool, torch.nn.AdaptiveAvgPool2d)
    assert m.classifier[6].out_features == 10


def test_registry_has_both_vggs():
    plain = build_model("vgg16_plain", 10)
    assert type(plain).__name__ == "VGGPlain"
    assert not any(isinstance(m, torch.nn.BatchNorm2d)
                   for m in plain.modules())
    bn = build_model("vgg16", 10)
    assert sum(isinstance(m, torch.nn.BatchNorm2d)
               for m in bn.modules()) == 13


def _flag(model):
    """fuse_model's flagging, without its check that the extension is
    built (the CPU fall-backs do not need it)."""
    for m in model.modules():
        if hasattr(m, "fused_ops"):
            m.fused_ops = True
    assert model.fused_ops and model.features[4].fused_ops
    return model


def test_flagged_model_on_cpu_equals_unflagged(monkeypatch):
    monkeypatch.delenv("KUBESHARE_BIAS_RELU", raising=False)
    monkeypatch.delenv("KUBESHARE_FUSED_POOL", raising=False)
    torch.manual_seed(0)
    model = vgg16_plain(num_classes=10).eval()
    x = torch.randn(1, 3, 32, 32)
    with torch.no_grad():
        want = model(x)
        assert not model.fused_ops
        _flag(model)
        assert torch.equal(model(x), want)
        monkeypatch.setenv("KUBESHARE_BIAS_RELU", "0")
        assert torch.equal(model(x), want)
    assert all(c._lowp_weight is None for c in model._lowp_convs)


def test_fused_walk_on_cpu(monkeypatch):
    """The walk itself, run on the CPU where every op falls back: 8 calls
    of bias_relu, 5 of bias_relu_pool, no pool module called, and the
    features of the stock modules up to fp32 rounding (the conv's own
    bias epilogue and a separate add round differently, so this is not
    exact: one rounding of an O(1) value per layer, 13 layers)."""
    monkeypatch.delenv("KUBESHARE_FUSED_POOL", raising=False)
    torch.manual_seed(0)
    model = _flag(vgg16_plain(num_classes=10).eval())
    x = torch.randn(1, 3, 32, 32)
    calls = {"bias_relu": 0, "bias_relu_pool": 0, "pool_module": 0}

    def count(name, fn):
        def wrapped(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(ops, "bias_relu", count("bias_relu", ops.bias_relu))
    monkeypatch.setattr(ops, "bias_relu_pool",
                        count("bias_relu_pool", ops.bias_relu_pool))
    hooks = [model.features[i].register_forward_hook(
        lambda *a: calls.update(pool_module=calls["pool_module"] + 1))
        for i in POOL_IDX]
    with torch.no_grad():
        got = model._fused_features(x, ops)
        assert calls == {"bias_relu": 8, "bias_relu_pool": 5,
                         "pool_module": 0}
        # KUBESHARE_FUSED_POOL=0: the pools stay modules
        monkeypatch.setenv("KUBESHARE_FUSED_POOL", "0")
        got2 = model._fused_features(x, ops)
        assert calls == {"bias_relu": 21, "bias_relu_pool": 5,
                         "pool_module": 5}
        for h in hooks:
            h.remove()
        want = model.features(x)
    assert torch.equal(got, got2)
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6)


def test_bench_worker_parser_accepts_vgg16_plain(monkeypatch):
    """main() parses first; an unknown model exits with status 2 there.
    The next thing main() does is import the tuning module: stop it at
    that point."""
    from kubeshare_amd import bench_worker

    class Parsed(Exception):
        pass

    import kubeshare_amd.utils.tuning as tuning

    def stop():
        raise Parsed

    monkeypatch.setattr(tuning, "apply_miopen_tuning", stop)
    monkeypatch.setattr(sys, "argv", ["bench_worker", "--model",
                                      "vgg16_plain", "--device", "cpu"])
    with pytest.raises(Parsed):
        bench_worker.main()
    monkeypatch.setattr(sys, "argv", ["bench_worker", "--model",
                                      "vgg19_plain", "--device", "cpu"])
    with pytest.raises(SystemExit):
        bench_worker.main()
