"""Multi-tensor weight casts (ops/hip/cast.hip) and their wiring into the
fused ResNet: one launch casts every conv weight to bf16 in forward, one
casts every weight gradient back in backward.

The cast is exact by construction (round-to-nearest-even with torch's
NaN rule one way, a 16-bit shift the other), so the unit tests compare
bit patterns with torch's own .to(). In the model tests the conv weight
gradients are only checked for dtype, shape and strides: MIOpen's
weight-gradient kernels accumulate with atomics and are not run-to-run
reproducible (see bench_worker.dump_outputs)."""
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

FN = "CastWeightsFn"

# f32 bit patterns: signed zeros, denormals, infinities, NaNs whose
# payload sits only in the low mantissa bits (a plain "add 0x7fff and
# shift" turns those into inf), quiet NaNs, exact rounding ties to even
# in both directions and their neighbours, and the finite values around
# the overflow to inf
PATTERNS = [
    0x00000000, 0x80000000,
    0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00008000, 0x00018000,
    0x7f800000, 0xff800000,
    0x7f800001, 0xff800001, 0x7f80ffff, 0xff80ffff, 0x7f808000,
    0x7fc00000, 0xffc00000, 0x7fffffff, 0xffffffff, 0x7fc00001,
    0x3f808000, 0x3f818000, 0x3f807fff, 0x3f808001, 0x3f817fff, 0x3f818001,
    0xbf808000, 0xbf818000,
    0x7f7fffff, 0xff7fffff, 0x7f7f8000, 0x7f7f7fff, 0x7f7f8001, 0x7f7e8000,
]


def _bits(t):
    return t.view(torch.int16)


def _pattern_tensor():
    g = torch.Generator().manual_seed(0)
    rnd = torch.randint(-2 ** 31, 2 ** 31, (5000,), generator=g,
                        dtype=torch.int64)
    fixed = torch.tensor(PATTERNS, dtype=torch.int64)
    fixed = torch.where(fixed >= 2 ** 31, fixed - 2 ** 32, fixed)
    return torch.cat([fixed, rnd]).to(torch.int32).cuda().view(torch.float32)


def _unit_inputs():
    g = torch.Generator(device="cuda").manual_seed(1)

    def rn(*shape):
        return torch.randn(shape, device="cuda", generator=g)

    base = rn(20001)
    odd = base.narrow(0, 1, 20000)  # 4 bytes past a 16-byte boundary
    assert odd.data_ptr() % 16 == 4
    ws = [rn(1), rn(3),
          rn(64, 3, 7, 7).contiguous(memory_format=torch.channels_last),
          rn(2048, 512, 1, 1), odd, _pattern_tensor()]
    # more tensors than one launch's argument table holds (128)
    ws += [rn(1 + 37 * i % 300) for i in range(140)]
    return ws


def test_cast_multi_matches_torch_bitwise_both_ways():
    ws = [w.requires_grad_() for w in _unit_inputs()]
    outs = ops.cast_weights_bf16(ws)
    assert len(outs) == len(ws)
    for w, o in zip(ws, outs):
        ref = w.detach().to(torch.bfloat16)
        assert o.dtype == torch.bfloat16 and o.shape == w.shape
        assert o.stride() == ref.stride() == w.stride()
        assert torch.equal(_bits(o), _bits(ref))
    assert outs[2].is_contiguous(memory_format=torch.channels_last)

    # backward: bf16 gradients with the outputs' strides; every third
    # output takes no part, so its weight's gradient is None
    g = torch.Generator(device="cuda").manual_seed(2)
    used = [i for i in range(len(ws)) if i % 3 != 1]
    gouts = []
    for i in used:
        gr = torch.empty_like(outs[i])
        gr.copy_(torch.randn(outs[i].shape, device="cuda", generator=g))
        gouts.append(gr)
    # the pattern tensor's own bf16 image as its gradient: every bf16
    # class (zeros, denormals, inf, NaN) through the widening cast
    pi = 5
    assert pi in used
    gouts[used.index(pi)] = outs[pi].detach().clone()
    grads = torch.autograd.grad([outs[i] for i in used], ws, gouts,
                                allow_unused=True)
    torch.cuda.synchronize()
    for i, gw in enumerate(grads):
        if i not in used:
            assert gw is None
            continue
        gin = gouts[used.index(i)]
        assert gw.dtype == torch.float32 and gw.shape == ws[i].shape
        assert gw.stride() == gin.stride()
        assert torch.equal(gw.view(torch.int32),
                           gin.float().view(torch.int32))


def test_backward_passes_f32_and_none_through():
    fn = ops._cast_weights_autograd()
    g16 = torch.randn(5, 4, device="cuda").to(torch.bfloat16)
    g32 = torch.randn(7, device="cuda")
    out = fn.backward(None, g16, None, g32)
    assert out[1] is None
    assert out[2] is g32
    assert out[0].dtype == torch.float32 and torch.equal(out[0], g16.float())
    assert fn.backward(None, None, None) == (None, None)


def test_extension_entry_points_none_and_non_dense():
    ext = ops._load()
    w = torch.randn(6, 10, device="cuda")
    sparse = w[:, ::2]  # not dense: goes through Tensor.to
    assert not sparse.is_contiguous()
    out = ext.cast_f32_to_bf16_multi([w, None, sparse])
    assert out[1] is None
    assert torch.equal(out[0], w.to(torch.bfloat16))
    assert torch.equal(out[2], sparse.to(torch.bfloat16))
    back = ext.cast_bf16_to_f32_multi([out[0], None, out[2][:, ::2]])
    assert back[1] is None
    assert torch.equal(back[0], out[0].float())
    assert torch.equal(back[2], out[2][:, ::2].float())
    assert ext.cast_f32_to_bf16_multi([]) == []


def test_cast_is_hipgraph_capturable():
    """Addresses ride in the kernel arguments; a captured cast re-reads
    the (static) sources on replay."""
    srcs = [torch.randn(n, device="cuda") for n in (5, 9000, 64)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        ops.cast_weights_bf16(srcs)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        outs = ops.cast_weights_bf16(srcs)
    for t in srcs:
        t.copy_(torch.randn_like(t))
    graph.replay()
    torch.cuda.synchronize()
    for t, o in zip(srcs, outs):
        assert torch.equal(o, t.to(torch.bfloat16))


# ----------------------------------------------------------- the model
def _conv_weights(model):
    return [p for p in model.parameters() if p.dim() == 4]


def _graph_nodes(root):
    seen, stack = set(), [root]
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        stack.extend(n for n, _ in fn.next_functions)
    return seen


def _resnet18_step(lowp):
    """One fused resnet18 forward + backward under bf16 autocast from a
    fixed seed; returns what the tests compare."""
    from kubeshare_amd.models import resnet18
    from kubeshare_amd.utils.tuning import apply_miopen_tuning
    apply_miopen_tuning()
    old_env = os.environ.get("KUBESHARE_LOWP_WEIGHTS")
    old_det = torch.backends.cudnn.deterministic
    os.environ["KUBESHARE_LOWP_WEIGHTS"] = lowp
    # as in test_bn_fork_gpu: MIOpen's default solver choice is not
    # reproducible at this size, so pin its deterministic solvers
    torch.backends.cudnn.deterministic = True
    try:
        torch.manual_seed(0)
        model = ops.fuse_model(resnet18(num_classes=10)).cuda().to(
            memory_format=torch.channels_last)
        g = torch.Generator(device="cuda").manual_seed(3)
        x = torch.randn(2, 3, 64, 64, device="cuda", generator=g).contiguous(
            memory_format=torch.channels_last)
        target = torch.tensor([1, 7], device="cuda")
        with torch.autocast("cuda", dtype=torch.bfloat16):
            logits = model(x)
            loss = F.cross_entropy(logits, target)
        nodes = _graph_nodes(loss.grad_fn)
        convw = {id(p) for p in _conv_weights(model)}
        feeders = []  # names of the nodes feeding a conv weight's grad
        for fn in nodes:
            for nxt, _ in fn.next_functions:
                if nxt is not None and nxt.name().endswith("AccumulateGrad") \
                        and id(nxt.variable) in convw:
                    feeders.append(fn.name())
        loss.backward()
        torch.cuda.synchronize()
        return dict(
            model=model, logits=logits.detach(),
            names=[fn.name() for fn in nodes], feeders=feeders,
            staged_after=[m._lowp_weight for m in model._lowp_convs])
    finally:
        torch.backends.cudnn.deterministic = old_det
        if old_env is None:
            os.environ.pop("KUBESHARE_LOWP_WEIGHTS", None)
        else:
            os.environ["KUBESHARE_LOWP_WEIGHTS"] = old_env


@pytest.fixture(scope="module")
def runs():
    return {flag: _resnet18_step(flag) for flag in ("1", "0")}


def test_routing_one_cast_node_replaces_the_per_weight_copies(runs):
    on, off = runs["1"], runs["0"]
    nconv = len(_conv_weights(on["model"]))
    assert nconv == 20 and len(on["model"]._lowp_convs) == nconv
    assert sum(FN in n for n in on["names"]) == 1
    assert len(on["feeders"]) == nconv
    assert all(FN in n for n in on["feeders"]), on["feeders"]
    assert not any("ToCopyBackward" in n for n in on["feeders"])
    # the staged references are gone once forward has returned
    assert all(w is None for w in on["staged_after"])

    assert not any(FN in n for n in off["names"])
    assert len(off["feeders"]) == nconv
    assert all(n == "ToCopyBackward0" for n in off["feeders"]), off["feeders"]


def test_staging_on_equals_off(runs):
    on, off = runs["1"], runs["0"]
    assert torch.equal(on["logits"], off["logits"])
    p_on = dict(on["model"].named_parameters())
    p_off = dict(off["model"].named_parameters())
    assert p_on.keys() == p_off.keys()
    checked = 0
    for name, p in p_on.items():
        q = p_off[name]
        assert p.grad is not None and q.grad is not None, name
        assert p.grad.dtype == q.grad.dtype == torch.float32, name
        assert p.grad.shape == q.grad.shape == p.shape, name
        assert p.grad.stride() == q.grad.stride(), name
        if p.dim() == 4:
            assert torch.isfinite(p.grad).all(), name
            continue
        assert torch.equal(p.grad, q.grad), name
        checked += 1
    assert checked == 20 * 2 + 2  # BN weights and biases, fc weight + bias


def test_staging_under_no_grad(monkeypatch):
    from kubeshare_amd.models import resnet18
    torch.manual_seed(0)
    model = ops.fuse_model(resnet18(num_classes=10)).cuda().to(
        memory_format=torch.channels_last)
    x = torch.randn(2, 3, 64, 64, device="cuda").contiguous(
        memory_format=torch.channels_last)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    outs = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("KUBESHARE_LOWP_WEIGHTS", flag)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            outs[flag] = model(x)
        assert outs[flag].grad_fn is None
        assert all(m._lowp_weight is None for m in model._lowp_convs)
    assert torch.equal(outs["1"], outs["0"])


def test_fp32_and_cpu_use_the_stock_path(monkeypatch):
    from kubeshare_amd.models import resnet18
    monkeypatch.delenv("KUBESHARE_LOWP_WEIGHTS", raising=False)
    torch.manual_seed(0)
    # fp32, no autocast, on the GPU: nothing is staged
    model = ops.fuse_model(resnet18(num_classes=10)).cuda().to(
        memory_format=torch.channels_last)
    x = torch.randn(2, 3, 64, 64, device="cuda").contiguous(
        memory_format=torch.channels_last)
    loss = model(x).float().sum()
    names = [fn.name() for fn in _graph_nodes(loss.grad_fn)]
    assert not any(FN in n for n in names)
    loss.backward()
    assert all(p.grad is not None and p.grad.dtype == torch.float32
               and torch.isfinite(p.grad).all() for p in model.parameters())
    assert all(m._lowp_weight is None for m in model._lowp_convs)
    # CPU, unfused
    cpu = resnet18(num_classes=10)
    out = cpu(torch.randn(2, 3, 32, 32))
    assert out.shape == (2, 10)
    assert not any(FN in fn.name() for fn in _graph_nodes(out.grad_fn))
    assert all(m._lowp_weight is None for m in cpu._lowp_convs)
