"""ops.wrw_gemm_conv (ops/hip/wrw_gemm.hip) and its routing through
ops.conv2d_split(wgrad_gemm="conv") and KUBESHARE_WRW_GEMM=all.

Reference: torch.nn.grad.conv2d_weight in float64 on the CPU from the same
bf16 inputs. Bound, per element, with Q = N*Ho*Wo:
    |got - ref| <= 2^-8 * |ref| + Q * 2^-24 * conv2d_weight(|x|, |dy|)
one bf16 rounding plus the worst case of an f32 accumulation of Q terms in
any order. Neither term is measured."""
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
from torch.nn.grad import conv2d_weight  # noqa: E402

from kubeshare_amd import ops  # noqa: E402
from kubeshare_amd.utils.tuning import apply_miopen_tuning  # noqa: E402

apply_miopen_tuning()

BF16 = torch.bfloat16
CL = torch.channels_last
CFGS = [(3, 1, 1), (1, 2, 0), (3, 2, 1)]  # (kernel, stride, padding)
MIXED = (2, 24, 40, 5, 7)     # ragged groups, odd sizes, two images
SLICED = (1, 16, 16, 19, 27)  # stride 1: Q = 513, slices of 256, 256, 1
RAGGED = (1, 264, 520, 2, 2)  # row tiles, short strips, empty strips
# the last case with (1, 2, 0) is the only one that launches the 256x64 tile
CASES = [MIXED, (1, 8, 8, 1, 1), SLICED, (2, 16, 16, 6, 8), RAGGED,
         (1, 64, 64, 3, 3), (1, 64, 256, 3, 3)]


def _rand(shape, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(shape, device="cuda", generator=g).to(BF16).contiguous(
        memory_format=CL)


def _inputs(case, cfg):
    n, c, k, h, w = case
    ker, st, p = cfg
    ho, wo = (h + 2 * p - ker) // st + 1, (w + 2 * p - ker) // st + 1
    return _rand((n, c, h, w), 1), _rand((n, k, ho, wo), 2)


def _check(dw, x, dy, cfg, tag):
    """dw against the float64 reference and the bound above, on the CPU."""
    ker, st, p = cfg
    xd, dyd = x.double().cpu().contiguous(), dy.double().cpu().contiguous()
    shape = (dy.shape[1], x.shape[1], ker, ker)
    ref = conv2d_weight(xd, shape, dyd, st, p)
    bound = 2.0 ** -8 * ref.abs() + dy.numel() // dy.shape[1] * 2.0 ** -24 * \
        conv2d_weight(xd.abs(), shape, dyd.abs(), st, p)
    err = (dw.double().cpu() - ref).abs()
    print(f"{tag}: max err {err.max().item():g}, "
          f"max err/bound {(err / bound.clamp_min(1e-300)).max().item():g}")
    assert torch.isfinite(dw).all() and (err <= bound).all(), tag


def _ids(c):
    return "x".join(map(str, c))


@pytest.mark.parametrize("cfg", CFGS, ids=_ids)
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_values_and_layout_against_float64(case, cfg):
    n, c, k, h, w = case
    ker, st, p = cfg
    x, dy = _inputs(case, cfg)
    dw = ops.wrw_gemm_conv(x, dy, ker, st, p)
    torch.cuda.synchronize()
    assert dw.dtype == BF16 and dw.shape == (k, c, ker, ker)
    assert dw.is_contiguous(memory_format=CL)
    _check(dw, x, dy, cfg, f"{_ids(case)} {_ids(cfg)}")
    # one-hot dy[q, k] = (q == k % Q): dW[k, :, r, s] is exactly the x pixel
    # that tap (r, s) of output pixel k % Q reads, zeros in the padding
    ho, wo = dy.shape[2:]
    q = n * ho * wo
    at = torch.arange(k, device="cuda") % q
    hot = (at[None, :] == torch.arange(q, device="cuda")[:, None]).to(BF16)
    hot = hot.view(n, ho, wo, k).permute(0, 3, 1, 2)
    got = ops.wrw_gemm_conv(x, hot, ker, st, p)
    xp = F.pad(x, (p, p, p, p))
    ni, hi, wi = at // (ho * wo), at // wo % ho * st, at % wo * st
    want = torch.stack([torch.stack([xp[ni, :, hi + r, wi + s]
                                     for s in range(ker)], -1)
                        for r in range(ker)], -2)
    assert torch.equal(got, want)


@pytest.mark.parametrize("case", [MIXED, SLICED], ids=_ids)
def test_1x1_stride_1_is_wrw_gemm_1x1(case):
    x, dy = _inputs(case, (1, 1, 0))
    assert torch.equal(ops.wrw_gemm_conv(x, dy, 1, 1, 0),
                       ops.wrw_gemm_1x1(x, dy))
    # the plan counts the taps: 9 strips in 3 tiles of 64x256, 3 slices
    assert ops._load().wrw_gemm_plan(513, 16, 16, 9) == [64, 256, 3, 256]


@pytest.mark.parametrize("case", [SLICED, RAGGED], ids=_ids)
def test_same_bits_on_every_call_and_stream(case):
    x, dy = _inputs(case, (3, 1, 1))
    a = ops.wrw_gemm_conv(x, dy, 3, 1, 1)
    b = ops.wrw_gemm_conv(x, dy, 3, 1, 1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = ops.wrw_gemm_conv(x, dy, 3, 1, 1)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c)


def _split(x, w, dy, cfg, x_grad, mirror, **kw):
    x = x.detach().clone(memory_format=torch.preserve_format).requires_grad_(
        x_grad)
    w = w.detach().clone(memory_format=torch.preserve_format).requires_grad_()
    wm = ops.mirror_weights([w.detach()])[0] if mirror else None
    y = ops.conv2d_split(x, w, cfg[1], cfg[2], 1, 1, wm, **kw)
    y.backward(dy)
    assert ops._load().wgrad_pending()
    ops.wgrad_join()
    assert not ops._load().wgrad_pending()
    torch.cuda.synchronize()
    return y.detach(), x.grad, w.grad


@pytest.mark.parametrize("cfg,x_grad,mirror", [
    ((3, 1, 1), True, False), ((3, 1, 1), True, True),
    ((3, 2, 1), False, False)])
def test_through_conv2d_split(cfg, x_grad, mirror):
    x, dy = _inputs(MIXED, cfg)
    w = _rand((40, 24, cfg[0], cfg[0]), 3)
    y0, dx0, _ = _split(x, w, dy, cfg, x_grad, mirror)
    y, dx, dw = _split(x, w, dy, cfg, x_grad, mirror, wgrad_gemm="conv")
    assert torch.equal(y, y0)
    assert torch.equal(dx, dx0) if x_grad else dx is None and dx0 is None
    assert dw.dtype == BF16 and dw.shape == w.shape
    _check(dw, x, dy, cfg, f"conv2d_split {cfg} mirror={mirror}")


@pytest.mark.parametrize("cin,ker,dil", [(16, 5, 1), (16, 3, 2), (12, 3, 1)],
                         ids=["5x5", "dilation2", "C12"])
def test_conv2d_split_rejects_what_the_kernel_does_not_cover(cin, ker, dil):
    x = _rand((2, cin, 6, 6), 1)
    w = _rand((16, cin, ker, ker), 2)
    pad = dil * (ker // 2)
    assert not ops.wrw_gemm_conv_supported(x, w, 1, pad, dil)
    with pytest.raises(RuntimeError, match="wgrad_gemm"):
        ops.conv2d_split(x, w, 1, pad, dil, wgrad_gemm="conv")


# ------------------------------------------------------------ model level
def _model_grads(monkeypatch, value, record=None):
    """{parameter: gradient} of a small fused ResNet under
    KUBESHARE_WRW_GEMM=value (None: unset), MIOpen pinned as in
    test_wrw_gemm_gpu; `record` gets {name: (x, dy, cfg)} of every conv."""
    from kubeshare_amd.models.resnet import Bottleneck, ResNet
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    if value is None:
        monkeypatch.delenv("KUBESHARE_WRW_GEMM", raising=False)
    else:
        monkeypatch.setenv("KUBESHARE_WRW_GEMM", value)
    torch.manual_seed(0)
    model = ops.fuse_model(ResNet(Bottleneck, [1, 1, 1, 1], 10)).cuda().to(
        memory_format=CL)
    def hook(mod, inputs, out):
        out.register_hook(lambda g: record.__setitem__(
            mod.key, (inputs[0].detach().to(BF16), g.detach(), (
                mod.kernel_size[0], mod.stride[0], mod.padding[0]))))
    for name, m in model.named_modules():
        if record is not None and isinstance(m, torch.nn.Conv2d):
            m.key = name + ".weight"
            m.register_forward_hook(hook)
    x = torch.randn(2, 3, 32, 32, device="cuda").contiguous(memory_format=CL)
    with torch.autocast("cuda", dtype=BF16):
        loss = F.cross_entropy(model(x), torch.tensor([1, 7], device="cuda"))
    loss.backward()
    ops.wgrad_join()
    torch.cuda.synchronize()
    return {n: p.grad for n, p in model.named_parameters()}


def test_model_gradients_reproduce_and_stay_within_the_bound(monkeypatch):
    seen, asked, split = {}, [], ops.conv2d_split
    monkeypatch.setattr(ops, "conv2d_split", lambda *a: asked.append(a[-1])
                        or split(*a))
    on = _model_grads(monkeypatch, "all", seen)
    # 4 blocks of 3 convs and a downsample ask for the kernel, the stem not
    assert asked.count("conv") == 16 and asked.count(False) == 1
    again = _model_grads(monkeypatch, "all")
    off = _model_grads(monkeypatch, None)
    for name, g in on.items():
        assert torch.equal(g, again[name]), name
        if name != "conv1.weight" and name in seen:
            _check(g, *seen[name], name)
        else:
            assert torch.equal(g, off[name]), name
