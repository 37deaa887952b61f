"""Residual-join fork: bn_relu(..., fork=True) hands y out under two
autograd handles and its backward sums the two incoming gradients inside
bn_bwd_stats_kernel. Reference: the unforked backward fed g1 + g2 (the
bf16 add autograd would have run). Every result must be bit-identical."""
import copy
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
    (2, 8, 3, 3),        # tail loop only
    (2, 24, 5, 5),       # channel groups do not divide the block
    (3, 2048, 7, 7),
    # N*H*W*C/8 > 4*1024*512: the smallest size at which every lane runs
    # the four-row group loop (whose dscale rounding pattern differs
    # from the leftover-row loop's) and then the leftover-row loop
    (17, 256, 64, 64),
]


def _cl(shape, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(shape, device="cuda", generator=g).to(
        torch.bfloat16).contiguous(memory_format=torch.channels_last)


def _setup(shape):
    x = _cl(shape, 0).requires_grad_()
    res = _cl(shape, 1).requires_grad_()
    bn = torch.nn.BatchNorm2d(shape[1]).cuda()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
    return x, res, bn, _cl(shape, 2), _cl(shape, 3)


def _grads(outs, gouts, x, res, bn):
    """(dx, dres, dweight, dbias)"""
    return torch.autograd.grad(outs, [x, res, bn.weight, bn.bias], gouts)


def _assert_equal(got, ref):
    for name, a, b in zip(("dx", "dres", "dweight", "dbias"), got, ref):
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert torch.equal(a, b), name


@pytest.mark.parametrize("shape", SHAPES)
def test_forked_backward_equals_unforked_on_sum(shape):
    x, res, bn, g1, g2 = _setup(shape)
    y = ops.bn_relu(x, bn, res=res)
    ref = _grads([y], [g1 + g2], x, res, bn)
    ya, yb = ops.bn_relu(x, bn, res=res, fork=True)
    assert ya.data_ptr() == yb.data_ptr()  # one activation, two handles
    assert torch.equal(ya, y)
    got = _grads([ya, yb], [g1, g2], x, res, bn)
    torch.cuda.synchronize()
    _assert_equal(got, ref)


@pytest.mark.parametrize("which", [0, 1])
def test_one_gradient_none(which):
    """A forked output without a consumer (the network's last block)
    contributes no gradient: same as the unforked backward."""
    x, res, bn, g1, _ = _setup((2, 24, 5, 5))
    y = ops.bn_relu(x, bn, res=res)
    ref = _grads([y], [g1], x, res, bn)
    pair = ops.bn_relu(x, bn, res=res, fork=True)
    got = _grads([pair[which]], [g1], x, res, bn)
    _assert_equal(got, ref)


def test_second_gradient_not_channels_last_falls_back():
    shape = (2, 24, 5, 5)
    x, res, bn, g1, g2 = _setup(shape)
    g2_nchw = g2.contiguous()  # same values, NCHW strides
    assert not g2_nchw.is_contiguous(memory_format=torch.channels_last)
    y = ops.bn_relu(x, bn, res=res)
    ref = _grads([y], [g1 + g2], x, res, bn)
    ya, yb = ops.bn_relu(x, bn, res=res, fork=True)
    got = _grads([ya, yb], [g1, g2_nchw], x, res, bn)
    _assert_equal(got, ref)


def test_fork_without_residual():
    """fork on a BN without a residual input sums on the host side."""
    shape = (2, 24, 5, 5)
    x, _, bn, g1, g2 = _setup(shape)
    y = ops.bn_relu(x, bn)
    ref = torch.autograd.grad([y], [x, bn.weight, bn.bias], [g1 + g2])
    ya, yb = ops.bn_relu(x, bn, fork=True)
    got = torch.autograd.grad([ya, yb], [x, bn.weight, bn.bias], [g1, g2])
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


@pytest.mark.parametrize("block", ["Bottleneck", "BasicBlock"])
def test_block_tensor_in_tensor_out_pair_in_pair_out(block):
    from kubeshare_amd.models import resnet as R
    blk = getattr(R, block)(64, 16 if block == "Bottleneck" else 64)
    blk = blk.cuda().to(memory_format=torch.channels_last)
    blk.fused_ops = True
    x = _cl((2, 64, 8, 8), 4)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = blk(x)
        pair = blk((x, x))
    assert isinstance(y, torch.Tensor)
    assert isinstance(pair, tuple) and len(pair) == 2
    assert torch.equal(pair[0], y) and torch.equal(pair[1], y)


def test_small_resnet50_fork_on_off(monkeypatch):
    """Whole fused ResNet50, forward + backward, fork on vs off: equal
    loss, input gradient, BN gradients and fc gradients. Conv weight
    gradients stay out: MIOpen's weight-gradient solvers accumulate with
    atomics (see bench_worker.dump_outputs). At this size MIOpen's
    default solver choice is not reproducible from one forward pass to
    the next even with the fork off (losses 2.7598 / 2.7324 / 2.7578 in
    three identical runs), so the convolutions are pinned to MIOpen's
    deterministic solvers for the comparison."""
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
    for fork in ("1", "0"):
        monkeypatch.setenv("KUBESHARE_BN_FORK", fork)
        model = copy.deepcopy(base)
        x = x0.clone().requires_grad_()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = torch.nn.functional.cross_entropy(model(x), target)
        loss.backward()
        grads = {n: p.grad for n, p in model.named_parameters()
                 if p.dim() != 4}
        runs[fork] = (loss.detach(), x.grad, grads)
    torch.cuda.synchronize()
    (l1, gx1, gr1), (l0, gx0, gr0) = runs["1"], runs["0"]
    assert torch.equal(l1, l0)
    assert torch.equal(gx1, gx0)
    assert gr1.keys() == gr0.keys() and len(gr1) == 53 * 2 + 2
    for name in gr1:
        assert torch.equal(gr1[name], gr0[name]), name
