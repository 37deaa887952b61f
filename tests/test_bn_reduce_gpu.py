"""Coalesced BN partial reduce(+finalize) against the legacy reduce and
finalize kernels (legacy_reduce=True / KUBESHARE_BN_REDUCE=legacy).

The new kernel is a re-mapping of threads and launches: per channel it
adds the same block partials into the same 64 accumulators in the same
order and folds them with the same tree, and the forward finalize math
is one pinned sequence shared by both paths. So every result must be
bit-identical (torch.equal), and no tolerance is involved."""
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

SHAPES = [
    (2, 8, 3, 3),        # one stats block, C smaller than a channel tile
    (2, 24, 5, 5),       # CG does not divide the block
    (1, 520, 9, 9),      # C not a multiple of the tile, CG > 64
    (4, 64, 30, 30),     # 57 blocks: some of the 64 accumulators are empty
    (3, 2048, 7, 7),     # 74 blocks: uneven accumulators, the largest CG
    (8, 64, 40, 40),     # 200 blocks
    # the 1024-block cap, 16 terms per accumulator, grouped + leftover rows
    (17, 256, 64, 64),
]
VARIANTS = ["plain", "norelu", "residual", "residual_fork"]
MOMENTUM, EPS = 0.1, 1e-5


def _cl(shape, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(shape, device="cuda", generator=g).to(
        torch.bfloat16).contiguous(memory_format=torch.channels_last)


def _inputs(shape, variant):
    C = shape[1]
    g = torch.Generator(device="cuda").manual_seed(10)
    residual = variant.startswith("residual")
    return dict(
        x=_cl(shape, 0),
        res=_cl(shape, 1) if residual else None,
        dy=_cl(shape, 2),
        dy2=_cl(shape, 3) if variant == "residual_fork" else None,
        w=torch.rand(C, device="cuda", generator=g) + 0.5,
        b=torch.rand(C, device="cuda", generator=g) - 0.5,
        rmean=torch.randn(C, device="cuda", generator=g),
        rvar=torch.rand(C, device="cuda", generator=g) + 0.5,
        relu=variant != "norelu",
    )


def _run(inp, legacy):
    """Forward + backward through the extension entry points (the saved
    statistics are not visible through autograd)."""
    ext = ops._load()
    rmean, rvar = inp["rmean"].clone(), inp["rvar"].clone()
    y, mean, invstd = ext.bn_relu_fwd_train(
        inp["x"], inp["w"], inp["b"], rmean, rvar, MOMENTUM, EPS, inp["res"],
        inp["relu"], legacy)
    out = ext.bn_relu_bwd(inp["x"], y, inp["dy"], inp["w"], inp["b"], mean,
                          invstd, inp["res"] is not None, inp["relu"],
                          inp["dy2"], legacy)
    got = dict(y=y, save_mean=mean, save_invstd=invstd, running_mean=rmean,
               running_var=rvar, dx=out[0], dweight=out[1], dbias=out[2])
    if inp["res"] is not None:
        got["dres"] = out[3]
    return got


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_new_reduce_equals_legacy_bitwise(shape, variant):
    inp = _inputs(shape, variant)
    ref = _run(inp, True)
    got = _run(inp, False)
    torch.cuda.synchronize()
    assert got.keys() == ref.keys()
    assert ("dres" in got) == variant.startswith("residual")
    for name in ref:
        a, b = got[name], ref[name]
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert torch.isfinite(b.float()).all(), name
        assert torch.equal(a, b), name
    # the running statistics did move (momentum update applied once)
    assert not torch.equal(ref["running_mean"], inp["rmean"])
    assert not torch.equal(ref["running_var"], inp["rvar"])


def test_env_switch_reaches_the_autograd_path(monkeypatch):
    """KUBESHARE_BN_REDUCE is read in Python per call; through
    ops.bn_relu both settings give the same bits, running stats
    included."""
    shape = (4, 64, 30, 30)
    runs = {}
    for setting in (None, "legacy"):
        if setting is None:
            monkeypatch.delenv("KUBESHARE_BN_REDUCE", raising=False)
        else:
            monkeypatch.setenv("KUBESHARE_BN_REDUCE", setting)
        assert ops.bn_reduce_legacy() == (setting == "legacy")
        x = _cl(shape, 0).requires_grad_()
        res = _cl(shape, 1).requires_grad_()
        torch.manual_seed(0)
        bn = torch.nn.BatchNorm2d(shape[1]).cuda()
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.5, 0.5)
        ya, yb = ops.bn_relu(x, bn, res=res, fork=True)
        grads = torch.autograd.grad(
            [ya, yb], [x, res, bn.weight, bn.bias],
            [_cl(shape, 2), _cl(shape, 3)])
        runs[setting] = (ya.detach(), bn.running_mean.clone(),
                         bn.running_var.clone()) + tuple(grads)
    torch.cuda.synchronize()
    for a, b in zip(runs[None], runs["legacy"]):
        assert torch.equal(a, b)
