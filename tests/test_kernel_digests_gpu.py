"""Bit-for-bit digests of the fused NHWC bf16 ops against a recorded
commit.

Most GPU tests here compare one of these kernels with another of them
(join against composition, mask against y, tile reduce against legacy) or
with torch under a tolerance, so a change that moves both sides the same
way passes them. This file pins the bits themselves: every op runs on
fixed inputs and the SHA-256 of each result's raw bytes (logical order:
NCHW for activations) must equal tests/golden/kernel_digests.json. The
kernels have no atomics and a fixed summation order, so a build
reproduces its own digests run after run; there is no tolerance and no
excluded case, and a case missing from the golden file fails.

The golden file is written by a checkout of the commit it names, never
by the code under test:

    python tests/test_kernel_digests_gpu.py --write [--commit <hash>]

Everything digested per case: the outputs, every tensor the autograd
node saved (mean/invstd, window codes, the ReLU mask bytes or y), the
gradients of the inputs and parameters, and the running statistics after
the step.

Shapes, the smallest that reach every path of the row walk, the block
partials and the pool window code:
  (2, 8, 7, 9)         C/8 = 1; odd H and W, so (3, 2, 1) windows hang
                       into the padding and with (2, 2, 0) the last row
                       belongs to no window
  (3, 24, 10, 6)       C/8 = 3 divides neither 512 nor 256: tail threads
                       idle
  (1, 2048, 4, 4)      C/8 = 256: one pixel per 256-thread block, two
                       rows per 512-thread block
  (1, 24, 1181, 1181)  1,394,761 rows > 4 * 2048 * (512 // 3) =
                       1,392,640: the unrolled body and then the
                       remainder loop run even under the 2048-block cap
                       of the apply kernels (bn_geom_of); the backward
                       stats kernels (1024 blocks) make two unrolled
                       passes of four rows plus a remainder and
                       bn_stats_kernel one pass of eight plus a
                       remainder, all with idle tail threads
"""
import contextlib
import functools
import hashlib
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    if __name__ == "__main__":
        sys.exit("no GPU")
    pytest.skip("no GPU", allow_module_level=True)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from kubeshare_amd import ops  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden", "kernel_digests.json")

SHAPES = [(2, 8, 7, 9), (3, 24, 10, 6), (1, 2048, 4, 4),
          (1, 24, 1181, 1181)]
POOLS = [(3, 2, 1), (2, 2, 0)]


# ----------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def _act(shape, seed):
    """Normal-valued channels-last bf16 on the GPU from a seeded CPU
    generator; shared between cases and never written to."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(shape, generator=g).to(torch.bfloat16)
    return t.cuda().contiguous(memory_format=torch.channels_last)


@pytest.fixture(scope="module", autouse=True)
def _release_inputs():
    """The shared inputs (67 MB each at the large shape) go when this
    module's tests are done."""
    yield
    _act.cache_clear()
    torch.cuda.empty_cache()


def _leaf(shape, seed):
    return _act(shape, seed).detach().requires_grad_()


def _vec(C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(C, generator=g), torch.rand(C, generator=g)


def _bn(C, seed, train=True):
    """BatchNorm2d whose weight has negative and exactly-zero channels
    and whose running statistics are not the initial ones."""
    n, u = _vec(C, seed)
    n2, u2 = _vec(C, seed + 1)
    bn = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(n)
        bn.weight[::3] = 0.0
        bn.bias.copy_(u - 0.5)
        bn.running_mean.copy_(0.1 * n2)
        bn.running_var.copy_(u2 + 0.5)
    bn = bn.cuda()
    return bn.train() if train else bn.eval()


def _bias(C, seed):
    """Centred, so that about half of relu(x + b) is zero."""
    n, _ = _vec(C, seed)
    return (0.25 * n).cuda().requires_grad_()


def _pooled(shape, cfg):
    k, s, p = cfg
    N, C, H, W = shape
    return (N, C, (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1)


@contextlib.contextmanager
def _env(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


# ---------------------------------------------------------------- digests
def _sha(t):
    t = t.detach().contiguous().cpu()
    h = hashlib.sha256(f"{t.dtype} {tuple(t.shape)} ".encode())
    h.update(t.reshape(-1).view(torch.uint8).numpy())
    return h.hexdigest()


def _run(out, grads, leaves, bns=()):
    """Digest the outputs and saved tensors of `out`, run its backward
    with `grads` (one per output) and digest the gradients of `leaves`
    and the parameters and running statistics of `bns`."""
    outs = out if isinstance(out, tuple) else (out,)
    d = {"y": _sha(outs[0])}
    if grads:
        for i, t in enumerate(outs[0].grad_fn.saved_tensors):
            d[f"saved{i}"] = _sha(t)
        torch.autograd.backward(list(outs), list(grads))
        for name, t in leaves.items():
            d[f"d{name}"] = _sha(t.grad)
    for i, bn in enumerate(bns):
        if grads:
            d[f"dweight{i}"] = _sha(bn.weight.grad)
            d[f"dbias{i}"] = _sha(bn.bias.grad)
        d[f"running_mean{i}"] = _sha(bn.running_mean)
        d[f"running_var{i}"] = _sha(bn.running_var)
    torch.cuda.synchronize()
    return d


def _bn_relu(shape, res, relu, fork, mask):
    x = _leaf(shape, 1)
    leaves = {"x": x}
    if res:
        leaves["res"] = _leaf(shape, 2)
    bn = _bn(shape[1], 10)
    # bn_relu's accepted inputs are bn_join_supported's, per tensor
    assert ops.bn_join_supported(x, x)
    with _env("KUBESHARE_BN_MASK", mask):
        out = ops.bn_relu(x, bn, res=leaves.get("res"), relu=relu, fork=fork)
        # a forked op gets two different gradients
        grads = [_act(shape, 3)] + ([_act(shape, 4)] if fork else [])
        return _run(out, grads, leaves, [bn])


def _bn_relu_eval(shape, res, relu):
    bn = _bn(shape[1], 10, train=False)
    # bn_relu's accepted inputs are bn_join_supported's, per tensor
    assert ops.bn_join_supported(_act(shape, 1), _act(shape, 2))
    with torch.no_grad():
        out = ops.bn_relu(_act(shape, 1), bn,
                          res=_act(shape, 2) if res else None, relu=relu)
    return _run(out, None, {}, [bn])


def _bn_join(shape, fork, mask):
    leaves = {"x": _leaf(shape, 1), "x_d": _leaf(shape, 2)}
    bn, bn_d = _bn(shape[1], 10), _bn(shape[1], 20)
    assert ops.bn_join_supported(leaves["x"], leaves["x_d"])
    with _env("KUBESHARE_BN_MASK", mask):
        out = ops.bn_join(leaves["x"], bn, leaves["x_d"], bn_d, fork=fork)
        grads = [_act(shape, 3)] + ([_act(shape, 4)] if fork else [])
        return _run(out, grads, leaves, [bn, bn_d])


def _max_pool(shape, cfg):
    x = _leaf(shape, 1)
    assert ops.max_pool_supported(x, *cfg)
    out = ops.max_pool_nhwc(x, *cfg)
    return _run(out, [_act(_pooled(shape, cfg), 5)], {"x": x})


def _bn_relu_pool(shape, cfg, train):
    bn = _bn(shape[1], 10, train=train)
    assert ops.bn_relu_pool_supported(_act(shape, 1), *cfg)
    if not train:
        with torch.no_grad():
            out = ops.bn_relu_pool(_act(shape, 1), bn, *cfg)
        return _run(out, None, {}, [bn])
    x = _leaf(shape, 1)
    out = ops.bn_relu_pool(x, bn, *cfg)
    return _run(out, [_act(_pooled(shape, cfg), 5)], {"x": x}, [bn])


def _bias_relu(shape):
    leaves = {"x": _leaf(shape, 1), "b": _bias(shape[1], 30)}
    assert ops.bias_relu_supported(leaves["x"])
    out = ops.bias_relu(leaves["x"], leaves["b"])
    return _run(out, [_act(shape, 3)], leaves)


def _bias_relu_pool(shape, cfg):
    leaves = {"x": _leaf(shape, 1), "b": _bias(shape[1], 30)}
    assert ops.bias_relu_pool_supported(leaves["x"], *cfg)
    out = ops.bias_relu_pool(leaves["x"], leaves["b"], *cfg)
    return _run(out, [_act(_pooled(shape, cfg), 5)], leaves)


def _ops():
    """(name, function of the shape) for every op and variant."""
    yield "bias_relu", _bias_relu
    # the backward's residual path requires the ReLU variant, and only
    # that path reads the mask or y: KUBESHARE_BN_MASK=0 is run there
    for res, relu, mask in ((0, 1, "1"), (0, 0, "1"), (1, 1, "1"),
                            (1, 1, "0")):
        for fork in (0, 1):
            yield (f"bn_relu-res{res}-relu{relu}-fork{fork}-mask{mask}",
                   functools.partial(_bn_relu, res=bool(res),
                                     relu=bool(relu), fork=bool(fork),
                                     mask=mask))
    for res, relu in ((0, 1), (0, 0), (1, 1), (1, 0)):
        yield (f"bn_relu_eval-res{res}-relu{relu}",
               functools.partial(_bn_relu_eval, res=bool(res),
                                 relu=bool(relu)))
    for mask in ("1", "0"):
        for fork in (0, 1):
            yield (f"bn_join-fork{fork}-mask{mask}",
                   functools.partial(_bn_join, fork=bool(fork), mask=mask))
    for cfg in POOLS:
        tag = "".join(map(str, cfg))
        yield f"max_pool-{tag}", functools.partial(_max_pool, cfg=cfg)
        yield (f"bn_relu_pool-{tag}",
               functools.partial(_bn_relu_pool, cfg=cfg, train=True))
        yield (f"bn_relu_pool_eval-{tag}",
               functools.partial(_bn_relu_pool, cfg=cfg, train=False))
        yield (f"bias_relu_pool-{tag}",
               functools.partial(_bias_relu_pool, cfg=cfg))


CASES = {f"{name}-{'x'.join(map(str, shape))}":
         functools.partial(fn, shape)
         for shape in SHAPES for name, fn in _ops()}


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", list(CASES))
def test_digest(case):
    want = _golden()["digests"]
    assert case in want, f"{case} is missing from {GOLDEN}"
    got = CASES[case]()
    diff = sorted(k for k in set(got) | set(want[case])
                  if got.get(k) != want[case].get(k))
    assert not diff, (f"{case}: {diff} differ from commit "
                      f"{_golden()['commit']}")


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true", required=True)
    ap.add_argument("--commit", default=None,
                    help="hash of the checked-out commit that writes "
                         "(default: git rev-parse HEAD)")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    if args.commit is None:
        import subprocess
        args.commit = subprocess.run(
            ["git", "-C", REPO, "rev-parse", "HEAD"], check=True,
            capture_output=True, text=True).stdout.strip()
    digests = {case: fn() for case, fn in CASES.items()}
    with open(args.out, "w") as f:
        json.dump({"commit": args.commit, "digests": digests}, f, indent=1,
                  sort_keys=True)
        f.write("\n")
    print(f"{len(digests)} cases -> {args.out}")
