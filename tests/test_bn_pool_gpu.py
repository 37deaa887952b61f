"""The fused BN+ReLU+max-pool op (ops.bn_relu_pool, ops/hip/bn_pool.hip)
on the GPU.

Oracle for the bit-exact checks: the composition
ops.max_pool_nhwc(ops.bn_relu(x, bn), ...) on a deep copy of the same
bn. The fused forward launches the composition's own statistics kernels
and pushes every window value through its apply expression, so y, the
running statistics and the saved mean / invstd are the same bits.

Backward: the two paths are compared through a float64 evaluation, on
the CPU, of the very quantity both compute (see _f64_reference). The
fused kernels keep the composition's launch geometry, so every lane
visits the same rows in the same order and in the same groups of four:
dbias (pure f32 adds of identical terms) is asserted bit-equal.

Each error-ratio case prints one JSON line (pytest -s shows them)."""
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

CFG_321 = (3, 2, 1)
CFG_220 = (2, 2, 0)
FN = "BNReLUMaxPoolNHWCFn"
# Grid formula of the backward kernels (bn_geom_of): 512-thread blocks of
# 512/(C/8) rows, at most 1024 (stats) / 2048 (apply) of them,
# grid-stride in groups of 4 rows. With C = 8 a block is 512 rows, so
# the apply kernel's unrolled body needs N*H*W > 4 * 2048 * 512 =
# 4,194,304 rows. 2049 * 2051 = 4,202,499 rows (67 MB of bf16):
#   stats kernel  stride 524,288: two passes of the unrolled body (all
#                 sub-batches of the group), then the remainder loop for
#                 the first 8,195 lanes;
#   apply kernel  stride 1,048,576: one pass of the unrolled body, then
#                 the remainder loop for the first 8,195 lanes.
# (The forward kernel has no loop: one output pixel per lane.) Both
# sizes are odd: the last 3/2/1 windows hang into the padding, the last
# 2/2/0 row and column belong to no window.
BIG = (1, 8, 2049, 2051)
CASES = [
    ((2, 8, 7, 9), CFG_321),
    ((3, 24, 10, 6), CFG_321),
    ((2, 64, 16, 16), CFG_321),
    ((1, 1536, 5, 5), CFG_321),
    ((1, 2048, 4, 4), CFG_321),
    (BIG, CFG_321),
    ((2, 8, 5, 7), CFG_220),
    ((3, 24, 9, 4), CFG_220),
    ((2, 64, 8, 8), CFG_220),
    ((1, 512, 14, 14), CFG_220),
    (BIG, CFG_220),
]
# pos      weight ~ U(0.5, 1.5), bias ~ U(-0.5, 0.5): about half the
#          pre-pool values are exact zeros, most windows tie
# mixed    weights of mixed sign, every third exactly 0: a negative
#          scale reverses the order, a zero scale ties whole windows
# allzero  bias = -100: everything is zero
KINDS = ["pos", "mixed", "allzero"]


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


def _input(shape, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return _cl(torch.randn(shape, device="cuda", generator=g)
               .to(torch.bfloat16))


def _bn(C, kind, seed=10):
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
        elif kind == "allzero":
            bn.bias.fill_(-100.0)
    return bn


def _upstream(y, seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return _cl(torch.randn(y.shape, device="cuda", generator=g)
               .to(torch.bfloat16))


def _composition(x, bn, cfg):
    return ops.max_pool_nhwc(ops.bn_relu(x, bn), *cfg)


def _both(x0, bn0, cfg, dy=None):
    """(fused, composition), each a dict with y, dx, dscale, dbias and
    the bn copy it ran on."""
    out = []
    for fn in (lambda x, bn: ops.bn_relu_pool(x, bn, *cfg),
               lambda x, bn: _composition(x, bn, cfg)):
        bn = copy.deepcopy(bn0)
        x = x0.detach().clone().requires_grad_()
        y = fn(x, bn)
        r = {"y": y, "bn": bn}
        if dy is not None:
            y.backward(dy)
            r.update(dx=x.grad, dscale=bn.weight.grad, dbias=bn.bias.grad)
        out.append(r)
    return out


def _f64_reference(x, dy, bn, cfg):
    """dbias, dscale (C) and dx (rows, C) in float64 on the CPU from x,
    the saved mean and invstd, and the routing and ReLU mask taken from
    the composition's own full-resolution y: the bf16 pool gradient that
    its gather kernel forms from the codes of that y, masked by y > 0."""
    ext = ops._load()
    C = x.shape[1]
    w32 = bn.weight.detach().float()
    b32 = bn.bias.detach().float()
    y_full, mean, invstd = ext.bn_relu_fwd_train(
        x.detach(), w32, b32, torch.zeros_like(w32), torch.ones_like(w32),
        bn.momentum, bn.eps, None, True, False)
    codes = ext.max_pool_nhwc_fwd(y_full, *cfg, True)[1]
    gp = ext.max_pool_nhwc_bwd(dy, codes, list(x.shape), *cfg)
    g = torch.where(y_full > 0, gp, torch.zeros_like(gp))

    def rows(t):
        return t.permute(0, 2, 3, 1).reshape(-1, C).cpu().double()

    G = rows(g)
    M = G.shape[0]
    xhat = rows(x.detach()).sub_(mean.cpu().double())\
        .mul_(invstd.cpu().double())
    dbias = G.sum(0)
    dscale = (G * xhat).sum(0)
    dx = xhat.mul_(dscale / M).neg_().add_(G).sub_(dbias / M)\
        .mul_((w32 * invstd).cpu().double())
    return dbias, dscale, dx, rows


def _err_ratios(fused, comp, ref):
    dbias, dscale, dx, rows = ref
    out = {}
    for name, want, conv in (("dbias", dbias, lambda t: t.cpu().double()),
                             ("dscale", dscale, lambda t: t.cpu().double()),
                             ("dx", dx, rows)):
        ef = (conv(fused[name]) - want).abs().max().item()
        ec = (conv(comp[name]) - want).abs().max().item()
        out[name] = (ef, ec)
    return out


def _assert_within_twice(errs, tag):
    line = {"bn_pool_err": tag}
    for name, (ef, ec) in errs.items():
        line[name + "_fused"] = ef
        line[name + "_composition"] = ec
        line[name + "_ratio"] = (ef / ec) if ec else (1.0 if ef == 0 else
                                                      float("inf"))
    print(json.dumps(line))
    for name, (ef, ec) in errs.items():
        # both are independent roundings of the same quantity; a wrong
        # window, a missing mask or a dropped row is off by orders of
        # magnitude
        assert ef <= 2 * ec, (name, ef, ec)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,cfg", CASES)
def test_matches_composition(shape, cfg, kind):
    x = _input(shape)
    bn0 = _bn(shape[1], kind)
    assert ops.bn_relu_pool_supported(x, *cfg)
    probe = _composition(x, copy.deepcopy(bn0), cfg)
    dy = _upstream(probe)
    fused, comp = _both(x, bn0, cfg, dy)
    torch.cuda.synchronize()

    y = fused["y"]
    # a silent fallback cannot pass
    assert FN in y.grad_fn.name()
    assert FN not in comp["y"].grad_fn.name()
    assert y.dtype == torch.bfloat16
    assert y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(y, comp["y"])
    for buf in ("running_mean", "running_var", "num_batches_tracked"):
        assert torch.equal(getattr(fused["bn"], buf),
                           getattr(comp["bn"], buf)), buf
    if kind == "allzero":
        assert not y.any()

    assert fused["dx"].dtype == torch.bfloat16
    assert fused["dx"].shape == x.shape
    errs = _err_ratios(fused, comp, _f64_reference(x, dy, bn0, cfg))
    _assert_within_twice(errs, {"shape": list(shape), "ksp": list(cfg),
                                "kind": kind})
    # the fused stats kernel keeps the composition's row order
    assert torch.equal(fused["dbias"], comp["dbias"])


@pytest.mark.parametrize("shape,cfg", CASES)
def test_backward_matches_fp32_reference(shape, cfg):
    """fp32 F.max_pool2d(relu(F.batch_norm(x32))) on the same bf16
    inputs, tolerances of test_ops_gpu.py's bn_relu test. Only the first
    parameter kind: ties at zero make the routing ambiguous against a
    reference whose pre-pool values differ in the last bit.

    The same holds for two positive window values that round to one
    bf16 value: the op (like the composition) sends the gradient to the
    first, the fp32 reference to the larger (with N(0, 1) inputs 3 of
    4320 elements of shape (3, 24, 10, 6) are then off by a whole
    gradient term). So x lives on a grid of multiples of 1/8 in
    [-3, 3]: equal x give equal values in both precisions (both take the
    first), distinct x differ before pooling by at least
    0.125 * 0.5 / std(x) ~ 0.06, twice the bf16 spacing of 2**-5 at the
    largest value (~5), so they stay distinct in bf16 and the routing of
    the reference is the op's."""
    C = shape[1]
    g = torch.Generator(device="cuda").manual_seed(2)
    x = _cl(torch.randn(shape, device="cuda", generator=g).mul(8).round()
            .clamp(-24, 24).div(8).to(torch.bfloat16)).requires_grad_()
    bn = _bn(C, "pos")
    y = ops.bn_relu_pool(x, bn, *cfg)
    assert FN in y.grad_fn.name()
    dy = _upstream(y)
    y.backward(dy)

    x32 = x.detach().float().requires_grad_()
    w32 = bn.weight.detach().clone().requires_grad_()
    b32 = bn.bias.detach().clone().requires_grad_()
    y32 = F.max_pool2d(torch.relu(F.batch_norm(
        x32, None, None, w32, b32, True, bn.momentum, bn.eps)), *cfg)
    y32.backward(dy.float())
    torch.cuda.synchronize()
    torch.testing.assert_close(y.detach().float(), y32.detach(),
                               rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(x.grad.float(), x32.grad,
                               rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(bn.weight.grad, w32.grad,
                               rtol=2e-2, atol=2e-1)
    torch.testing.assert_close(bn.bias.grad, b32.grad, rtol=2e-2, atol=2e-1)


@pytest.mark.parametrize("cfg", [CFG_321, CFG_220])
def test_nan_goes_where_the_composition_puts_it(cfg):
    shape = (1, 8, 6, 6)
    x = _input(shape, seed=3)
    with torch.no_grad():
        x[0, 5, 3, 2] = float("nan")
    bn0 = _bn(8, "pos")
    probe = _composition(x, copy.deepcopy(bn0), cfg)
    dy = torch.ones_like(probe)
    fused, comp = _both(x, bn0, cfg, dy)
    torch.cuda.synchronize()
    assert FN in fused["y"].grad_fn.name()
    # the batch statistics of channel 5 are NaN: so is all of it
    assert comp["y"].isnan().any() and not comp["y"].isnan().all()
    for name in ("y", "dx"):
        a, b = fused[name].detach(), comp[name].detach()
        assert torch.equal(a.isnan(), b.isnan()), name
        assert torch.equal(a[~a.isnan()], b[~b.isnan()]), name
    assert comp["dx"].isnan().any()


def test_autograd_keeps_no_full_resolution_activation():
    shape, cfg = (8, 64, 112, 112), CFG_321
    x = _input(shape, seed=4).requires_grad_()
    bn0 = _bn(64, "pos")

    def held(fn):
        bn = copy.deepcopy(bn0)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        y = fn(x, bn)
        torch.cuda.synchronize()
        return torch.cuda.memory_allocated() - before, y

    fused, y = held(lambda x, bn: ops.bn_relu_pool(x, bn, *cfg))
    assert FN in y.grad_fn.name()
    del y
    comp, y = held(lambda x, bn: _composition(x, bn, cfg))
    del y
    print(json.dumps({"bn_pool_held_bytes": {"fused": fused,
                                             "composition": comp,
                                             "x": x.numel() * 2}}))
    assert fused <= comp - 0.9 * x.numel() * 2, (fused, comp)


@pytest.mark.parametrize("cfg", [CFG_321, CFG_220])
@pytest.mark.parametrize("training", [True, False])
def test_no_grad_and_eval(cfg, training):
    x = _input((2, 64, 9, 9), seed=5).requires_grad_()
    bn0 = _bn(64, "mixed")
    with torch.no_grad():  # non-trivial running statistics
        bn0.running_mean.uniform_(-0.5, 0.5)
        bn0.running_var.uniform_(0.5, 1.5)
    bn0.train(training)
    a, b = copy.deepcopy(bn0), copy.deepcopy(bn0)
    with torch.no_grad():
        y = ops.bn_relu_pool(x, a, *cfg)
        y_ref = _composition(x, b, cfg)
    assert y.grad_fn is None and not y.requires_grad
    assert torch.equal(y, y_ref)
    assert torch.equal(a.running_mean, b.running_mean)
    assert torch.equal(a.running_var, b.running_var)
    # an input that needs no gradient takes the same code-free path
    for p in a.parameters():
        p.requires_grad_(False)
    y2 = ops.bn_relu_pool(x.detach(), a, *cfg)
    assert y2.grad_fn is None
    assert torch.equal(y2, y_ref)
    # the entry points allocate no codes tensor then
    ext = ops._load()
    w32, b32 = bn0.weight.detach(), bn0.bias.detach()
    rm, rv = bn0.running_mean.clone(), bn0.running_var.clone()
    assert len(ext.bn_relu_pool_fwd_eval(x.detach(), w32, b32, rm, rv,
                                         bn0.eps, *cfg)) == 1
    out = ext.bn_relu_pool_fwd_train(x.detach(), w32, b32, rm, rv,
                                     bn0.momentum, bn0.eps, *cfg, False)
    assert len(out) == 3
    out = ext.bn_relu_pool_fwd_train(x.detach(), w32, b32, rm, rv,
                                     bn0.momentum, bn0.eps, *cfg, True)
    assert len(out) == 4 and out[3].dtype == torch.uint8
    assert tuple(out[3].shape) == (2, y.shape[2], y.shape[3], 64)
    assert int(out[3].max()) < cfg[0] * cfg[0]


@pytest.mark.parametrize("training", [False, True])
def test_no_grad_forward_is_hipgraph_capturable(training):
    """One linear branch: warm up on a side stream (as GraphReplayServer
    does), capture, copy new data into the static input, replay."""
    cfg = CFG_321
    bn = _bn(64, "mixed").train(training)
    static_in = _input((2, 64, 12, 12), seed=7)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        for _ in range(3):
            ops.bn_relu_pool(static_in, bn, *cfg)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        static_out = ops.bn_relu_pool(static_in, bn, *cfg)
    new = _input((2, 64, 12, 12), seed=8) * 2 + 1
    static_in.copy_(new)
    eager_bn = copy.deepcopy(bn)
    graph.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        eager = ops.bn_relu_pool(_cl(new), eager_bn, *cfg)
    assert torch.equal(static_out, eager)
    assert torch.equal(bn.running_mean, eager_bn.running_mean)


def _fallback_case(name):
    g = torch.Generator(device="cuda").manual_seed(6)

    def rn(*shape):
        return torch.randn(shape, device="cuda", generator=g)

    bf = torch.bfloat16
    x, cfg = {
        "c12": (_cl(rn(2, 12, 9, 9).to(bf)), CFG_321),
        "fp32": (_cl(rn(2, 16, 9, 9)), CFG_321),
        "nchw": (rn(2, 16, 9, 9).to(bf), CFG_321),
        "k3s1p1": (_cl(rn(2, 16, 9, 9).to(bf)), (3, 1, 1)),
        "eval_grad": (_cl(rn(2, 16, 9, 9).to(bf)), CFG_321),
        "env": (_cl(rn(2, 16, 9, 9).to(bf)), CFG_321),
    }[name]
    return x, cfg


@pytest.mark.parametrize("name", ["c12", "fp32", "nchw", "k3s1p1",
                                  "eval_grad", "env"])
def test_fallbacks_run_the_composition(name, monkeypatch):
    monkeypatch.delenv("KUBESHARE_BN_POOL", raising=False)
    x, cfg = _fallback_case(name)
    bn0 = _bn(x.shape[1], "pos")
    if name == "eval_grad":
        bn0.eval()
    if name == "env":
        monkeypatch.setenv("KUBESHARE_BN_POOL", "0")
        assert not ops.bn_pool_enabled()
    supported = name in ("eval_grad", "env")
    assert ops.bn_relu_pool_supported(x, *cfg) == supported
    probe = _composition(x, copy.deepcopy(bn0), cfg)
    # ones: the eager pool backward sums with atomics, and sums of ones
    # are exact in any order
    dy = torch.ones_like(probe)
    fused, comp = _both(x, bn0, cfg, dy)
    assert FN not in fused["y"].grad_fn.name()
    assert fused["y"].grad_fn.name() == comp["y"].grad_fn.name()
    for key in ("y", "dx", "dscale", "dbias"):
        assert torch.equal(fused[key], comp[key]), key
    assert torch.equal(fused["bn"].running_mean, comp["bn"].running_mean)


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
def test_fused_models_route_through_the_fused_op(name, shape, monkeypatch):
    monkeypatch.delenv("KUBESHARE_FUSED_POOL", raising=False)
    monkeypatch.delenv("KUBESHARE_BN_POOL", raising=False)
    seen = _run_model(name, shape)
    assert all(FN in n for n in seen), seen
    monkeypatch.setenv("KUBESHARE_BN_POOL", "0")
    seen = _run_model(name, shape)
    assert all(n == "MaxPoolNHWCFnBackward" for n in seen), seen
    monkeypatch.delenv("KUBESHARE_BN_POOL")
    monkeypatch.setenv("KUBESHARE_FUSED_POOL", "0")
    seen = _run_model(name, shape)
    assert not any("MaxPoolNHWCFn" in n for n in seen), seen


def test_small_resnet50_bn_pool_on_off(monkeypatch):
    """Whole fused ResNet50, forward + backward, KUBESHARE_BN_POOL on vs
    off, convolutions pinned to MIOpen's deterministic solvers as in
    test_small_resnet50_fork_on_off. Loss, logits and every non-conv
    gradient other than bn1's are bit-equal: the stem is the last BN the
    backward pass reaches, so nothing else can differ. bn1's gradients
    are held to the float64-referenced bound of
    test_matches_composition."""
    from kubeshare_amd.models import resnet50
    from kubeshare_amd.utils.tuning import apply_miopen_tuning
    apply_miopen_tuning()
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    torch.manual_seed(0)
    base = ops.fuse_model(resnet50(num_classes=10)).cuda().to(
        memory_format=torch.channels_last)
    x0 = torch.randn(4, 3, 64, 64, device="cuda").contiguous(
        memory_format=torch.channels_last)
    target = torch.randint(0, 10, (4,), device="cuda")
    runs = {}
    for on in ("1", "0"):
        monkeypatch.setenv("KUBESHARE_BN_POOL", on)
        model = copy.deepcopy(base)
        stem = {}
        h1 = model.conv1.register_forward_hook(
            lambda mod, inp, out: stem.update(x=out.detach()))

        def pool_hook(mod, inp, out, stem=stem):
            stem.update(fn=out.grad_fn.name())
            out.register_hook(lambda g: stem.update(dy=g.detach()))

        h2 = model.maxpool.register_forward_hook(pool_hook)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            logits = model(x0)
            loss = F.cross_entropy(logits, target)
        loss.backward()
        h1.remove()
        h2.remove()
        grads = {n: p.grad for n, p in model.named_parameters()
                 if p.dim() != 4}
        runs[on] = (loss.detach(), logits.detach(), grads, stem)
    torch.cuda.synchronize()
    (l1, z1, g1, s1), (l0, z0, g0, s0) = runs["1"], runs["0"]
    assert FN in s1["fn"] and s0["fn"] == "MaxPoolNHWCFnBackward"
    assert torch.equal(l1, l0)
    assert torch.equal(z1, z0)
    stem_keys = ("bn1.weight", "bn1.bias")
    assert all(k in g1 for k in stem_keys)
    for k in g1:
        if k not in stem_keys:
            assert torch.equal(g1[k], g0[k]), k
    # the same x and dy reached the stem in both runs
    assert torch.equal(s1["x"], s0["x"]) and torch.equal(s1["dy"], s0["dy"])
    dbias, dscale, _, _ = _f64_reference(
        _cl(s0["x"]), _cl(s0["dy"]), base.bn1, CFG_321)
    errs = {}
    for name, key, want in (("dscale", "bn1.weight", dscale),
                            ("dbias", "bn1.bias", dbias)):
        errs[name] = ((g1[key].cpu().double() - want).abs().max().item(),
                      (g0[key].cpu().double() - want).abs().max().item())
    _assert_within_twice(errs, {"model": "resnet50", "tensor": "bn1"})
