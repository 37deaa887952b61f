"""The fused downsample join (ops.bn_join, ops/hip/bn_join.hip) on the
GPU: y = relu(bn(x) + bn_d(x_d)).

Oracle: the composition
ops.bn_relu(x, bn, res=ops.bn_relu(x_d, bn_d, relu=False), fork=fork) on
deep copies of the same two BNs. The fused forward launches the
composition's own statistics kernels and rounds the downsample branch to
bf16 where the composition stored it; the fused backward keeps the
composition's launch geometry, row order and groups of four and goes
through the same pinned expressions. Everything is therefore asserted
with torch.equal: y, both BNs' running buffers, dx, dx_d and both weight
and bias gradients. The bias gradient of the two BNs is one sum."""
import copy
import json
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

FN = "BNJoinFn"
# (1, 8, 2049, 2051): the only size at which the 2048-block apply kernels
# run their unrolled body (see BIG in test_bn_pool_gpu.py)
BIG = (1, 8, 2049, 2051)
SHAPES = [
    (2, 8, 3, 3),        # leftover-row loop only
    (2, 24, 5, 5),       # C/8 does not divide the block
    (3, 2048, 7, 7),     # largest C
    # every lane of the stats kernel runs one four-row group and some
    # run the leftover loop (reasoning in test_bn_fork_gpu.py)
    (17, 256, 64, 64),
]
CASES = [(s, k) for s in SHAPES for k in ("pos", "mixed")] + [(BIG, "pos")]
KEYS = ("y", "dx", "dx_d", "dscale", "dbias", "dscale_d", "dbias_d")


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


def _rand(shape, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return _cl(torch.randn(shape, device="cuda", generator=g)
               .to(torch.bfloat16))


def _bn(C, kind, seed):
    """pos: weight ~ U(0.5, 1.5), bias ~ U(-0.5, 0.5); mixed: weights of
    mixed sign, every third exactly 0 (as in test_bn_pool_gpu.py)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    bn = torch.nn.BatchNorm2d(C).cuda()
    with torch.no_grad():
        u = torch.rand(C, device="cuda", generator=g)
        v = torch.rand(C, device="cuda", generator=g)
        bn.weight.copy_(0.5 + u)
        bn.bias.copy_(v - 0.5)
        if kind == "mixed":
            bn.weight.copy_(torch.randn(C, device="cuda", generator=g))
            bn.weight[::3] = 0.0
    return bn


def _composition(x, bn, x_d, bn_d, fork=False):
    return ops.bn_relu(x, bn, res=ops.bn_relu(x_d, bn_d, relu=False),
                       fork=fork)


def _run(fn, x0, xd0, bn0, bnd0, fork, g1, g2):
    """One forward + backward of fn on fresh leaves and BN copies; g1 /
    g2 are the gradients of the two handles (None: no consumer)."""
    bn, bn_d = copy.deepcopy(bn0), copy.deepcopy(bnd0)
    x = x0.detach().clone().requires_grad_()
    x_d = xd0.detach().clone().requires_grad_()
    out = fn(x, bn, x_d, bn_d, fork=fork)
    if fork:
        y, y2 = out
        assert y2.data_ptr() == y.data_ptr()
        pairs = [(t, g) for t, g in ((y, g1), (y2, g2)) if g is not None]
    else:
        y = out
        pairs = [(y, g1)]
    torch.autograd.backward([t for t, _ in pairs], [g for _, g in pairs])
    return {"y": y.detach(), "fn": y.grad_fn.name(), "bn": bn, "bn_d": bn_d,
            "dx": x.grad, "dx_d": x_d.grad, "dscale": bn.weight.grad,
            "dbias": bn.bias.grad, "dscale_d": bn_d.weight.grad,
            "dbias_d": bn_d.bias.grad}


def _both(shape, kind="pos", fork=True, g1=True, g2=True, x_d=None,
          bns=None, seed=0):
    x = _rand(shape, seed)
    x_d = _rand(shape, seed + 1) if x_d is None else x_d
    bn0, bnd0 = bns or (_bn(shape[1], kind, 10), _bn(shape[1], kind, 11))
    g1 = _rand(shape, seed + 2) if g1 else None
    g2 = _rand(shape, seed + 3) if g2 else None
    fused = _run(ops.bn_join, x, x_d, bn0, bnd0, fork, g1, g2)
    comp = _run(_composition, x, x_d, bn0, bnd0, fork, g1, g2)
    torch.cuda.synchronize()
    return fused, comp


def _assert_bit_equal(fused, comp):
    for key in KEYS:
        assert fused[key].dtype == comp[key].dtype, key
        assert torch.equal(fused[key], comp[key]), key
    for which in ("bn", "bn_d"):
        for buf in ("running_mean", "running_var", "num_batches_tracked"):
            assert torch.equal(getattr(fused[which], buf),
                               getattr(comp[which], buf)), (which, buf)
    # one ordered sum of the same terms serves both BNs
    assert torch.equal(comp["dbias_d"], comp["dbias"])
    assert torch.equal(fused["dbias_d"], fused["dbias"])
    assert fused["dbias_d"].data_ptr() != fused["dbias"].data_ptr()


@pytest.mark.parametrize("shape,kind", CASES)
def test_matches_composition(shape, kind, monkeypatch):
    monkeypatch.delenv("KUBESHARE_BN_JOIN", raising=False)
    monkeypatch.delenv("KUBESHARE_BN_MASK", raising=False)
    fused, comp = _both(shape, kind)
    # a silent fallback cannot pass
    assert FN in fused["fn"] and FN not in comp["fn"]
    assert fused["y"].dtype == torch.bfloat16
    assert fused["y"].is_contiguous(memory_format=torch.channels_last)
    assert fused["dx"].shape == fused["dx_d"].shape == torch.Size(shape)
    _assert_bit_equal(fused, comp)


@pytest.mark.parametrize("shape", [(2, 24, 5, 5), (17, 256, 64, 64)])
@pytest.mark.parametrize("which", ["first", "second", "unforked"])
def test_one_gradient(shape, which, monkeypatch):
    """fork=True with each handle's gradient None in turn, and
    fork=False: the one-gradient kernels."""
    monkeypatch.delenv("KUBESHARE_BN_JOIN", raising=False)
    fork = which != "unforked"
    fused, comp = _both(shape, "mixed", fork=fork, g1=which != "first",
                        g2=which == "first")
    assert FN in fused["fn"] and FN not in comp["fn"]
    _assert_bit_equal(fused, comp)


def test_second_gradient_not_channels_last(monkeypatch):
    """A dy2 with NCHW strides is summed on the host side first, as in
    bn_relu_bwd."""
    monkeypatch.delenv("KUBESHARE_BN_JOIN", raising=False)
    shape = (2, 24, 5, 5)
    x, x_d = _rand(shape, 0), _rand(shape, 1)
    bn0, bnd0 = _bn(24, "pos", 10), _bn(24, "pos", 11)
    g1, g2 = _rand(shape, 2), _rand(shape, 3).contiguous()
    fused = _run(ops.bn_join, x, x_d, bn0, bnd0, True, g1, g2)
    comp = _run(_composition, x, x_d, bn0, bnd0, True, g1, g2)
    assert FN in fused["fn"]
    _assert_bit_equal(fused, comp)


def test_nan_goes_where_the_composition_puts_it(monkeypatch):
    monkeypatch.delenv("KUBESHARE_BN_JOIN", raising=False)
    shape = (2, 16, 5, 5)
    x_d = _rand(shape, 1)
    with torch.no_grad():
        x_d[1, 5, 3, 2] = float("nan")
    fused, comp = _both(shape, "pos", x_d=x_d)
    assert FN in fused["fn"]
    # the batch statistics of channel 5 are NaN: so is all of it
    assert comp["y"].isnan().any() and not comp["y"].isnan().all()
    assert comp["dx_d"].isnan().any()
    for name in ("y", "dx", "dx_d"):
        a, b = fused[name], comp[name]
        assert torch.equal(a.isnan(), b.isnan()), name
        assert torch.equal(a[~a.isnan()], b[~b.isnan()]), name


def _fallback_inputs(name):
    bf = torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(6)

    def rn(*shape):
        return torch.randn(shape, device="cuda", generator=g)

    if name == "fp32":
        return _cl(rn(2, 16, 5, 5)), _cl(rn(2, 16, 5, 5))
    if name == "c12":
        return _cl(rn(2, 12, 5, 5).to(bf)), _cl(rn(2, 12, 5, 5).to(bf))
    if name == "nchw":
        return rn(2, 16, 5, 5).to(bf), rn(2, 16, 5, 5).to(bf)
    return _cl(rn(2, 16, 5, 5).to(bf)), _cl(rn(2, 16, 5, 5).to(bf))


@pytest.mark.parametrize("name", ["fp32", "c12", "nchw", "eval", "env"])
def test_fallbacks_run_the_composition(name, monkeypatch):
    monkeypatch.delenv("KUBESHARE_BN_JOIN", raising=False)
    x, x_d = _fallback_inputs(name)
    C = x.shape[1]
    bn0, bnd0 = _bn(C, "pos", 10), _bn(C, "pos", 11)
    if name == "eval":
        for bn in (bn0, bnd0):
            with torch.no_grad():
                bn.running_mean.uniform_(-0.5, 0.5)
                bn.running_var.uniform_(0.5, 1.5)
            bn.eval()
    if name == "env":
        monkeypatch.setenv("KUBESHARE_BN_JOIN", "0")
        assert not ops.bn_join_enabled()
    assert ops.bn_join_supported(x, x_d) == (name in ("eval", "env"))
    g1 = torch.ones_like(x)
    fused = _run(ops.bn_join, x, x_d, bn0, bnd0, False, g1, None)
    comp = _run(_composition, x, x_d, bn0, bnd0, False, g1, None)
    assert FN not in fused["fn"]
    assert fused["fn"] == comp["fn"]
    for key in KEYS:
        assert torch.equal(fused[key], comp[key]), key
    for which in ("bn", "bn_d"):
        assert torch.equal(fused[which].running_mean,
                           comp[which].running_mean)


def test_autograd_does_not_keep_the_downsample_output(monkeypatch):
    monkeypatch.delenv("KUBESHARE_BN_JOIN", raising=False)
    shape = (8, 64, 56, 56)
    x = _rand(shape, 4).requires_grad_()
    x_d = _rand(shape, 5).requires_grad_()
    bn0, bnd0 = _bn(64, "pos", 10), _bn(64, "pos", 11)

    def held(fn):
        bn, bn_d = copy.deepcopy(bn0), copy.deepcopy(bnd0)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        y = fn(x, bn, x_d, bn_d)
        torch.cuda.synchronize()
        return torch.cuda.memory_allocated() - before, y

    fused, y = held(ops.bn_join)
    assert FN in y.grad_fn.name()
    del y
    comp, y = held(_composition)
    del y
    print(json.dumps({"bn_join_held_bytes": {"fused": fused,
                                             "composition": comp,
                                             "x": x.numel() * 2}}))
    assert fused <= comp - 0.9 * x.numel() * 2, (fused, comp)


def _run_model(name, batch):
    from kubeshare_amd.models import resnet18, resnet50
    from kubeshare_amd.models.resnet import BasicBlock, Bottleneck

    torch.manual_seed(0)
    model = {"resnet18": resnet18, "resnet50": resnet50}[name](
        num_classes=10)
    model = ops.fuse_model(model).cuda().to(
        memory_format=torch.channels_last)
    seen = []

    def hook(mod, inp, out):
        out = out[0] if isinstance(out, tuple) else out
        seen.append(out.grad_fn.name())

    hooks = [m.register_forward_hook(hook) for m in model.modules()
             if isinstance(m, (BasicBlock, Bottleneck))]
    x = _cl(torch.randn(batch, 3, 64, 64, device="cuda"))
    t = torch.randint(0, 10, (batch,), device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = F.cross_entropy(model(x), t)
    loss.backward()
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    assert torch.isfinite(loss).item()
    assert all(p.grad is not None and torch.isfinite(p.grad).all()
               for p in model.parameters())
    return seen


@pytest.mark.parametrize("name,blocks,joins", [("resnet18", 8, 3),
                                               ("resnet50", 16, 4)])
def test_fused_models_route_through_the_join(name, blocks, joins,
                                             monkeypatch):
    monkeypatch.delenv("KUBESHARE_BN_JOIN", raising=False)
    seen = _run_model(name, 2)
    assert len(seen) == blocks
    assert sum(FN in n for n in seen) == joins, seen
    assert all(FN in n or "BNReLUFn" in n for n in seen), seen
    monkeypatch.setenv("KUBESHARE_BN_JOIN", "0")
    seen = _run_model(name, 2)
    assert len(seen) == blocks and all("BNReLUFn" in n for n in seen), seen


def test_small_resnet50_join_on_off(monkeypatch):
    """Whole fused ResNet50, forward + backward, KUBESHARE_BN_JOIN on vs
    off, convolutions pinned to MIOpen's deterministic solvers as in
    test_small_resnet50_bn_pool_on_off. Loss, logits and every non-conv
    gradient are bit-equal."""
    from kubeshare_amd.models import resnet50
    from kubeshare_amd.utils.tuning import apply_miopen_tuning
    apply_miopen_tuning()
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    torch.manual_seed(0)
    base = ops.fuse_model(resnet50(num_classes=10)).cuda().to(
        memory_format=torch.channels_last)
    x0 = _cl(torch.randn(4, 3, 64, 64, device="cuda"))
    target = torch.randint(0, 10, (4,), device="cuda")
    runs = {}
    for on in ("1", "0"):
        monkeypatch.setenv("KUBESHARE_BN_JOIN", on)
        model = copy.deepcopy(base)
        names = []
        h = model.layer1[0].register_forward_hook(
            lambda mod, inp, out: names.append(
                (out[0] if isinstance(out, tuple) else out).grad_fn.name()))
        with torch.autocast("cuda", dtype=torch.bfloat16):
            logits = model(x0)
            loss = F.cross_entropy(logits, target)
        loss.backward()
        h.remove()
        grads = {n: p.grad for n, p in model.named_parameters()
                 if p.dim() != 4}
        runs[on] = (loss.detach(), logits.detach(), grads, names[0])
    torch.cuda.synchronize()
    (l1, z1, g1, n1), (l0, z0, g0, n0) = runs["1"], runs["0"]
    assert FN in n1 and FN not in n0
    assert torch.equal(l1, l0)
    assert torch.equal(z1, z0)
    assert len(g1) == len(g0) > 100
    for k in g1:
        assert torch.equal(g1[k], g0[k]), k
