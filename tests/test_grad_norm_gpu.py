"""hip/grad_norm.hip and ops.FusedSGD's clipping / LARS step against f64
references (norms at rtol 1e-5: a tree at most 300 roundings deep gives
1.8e-5 on a sum of squares, half of that on a norm; updates at rtol 1e-5
/ atol 1e-6) and bit for bit against the plain, eager and ungrouped step."""
import datetime
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

LR, MU, WD, ETA, EPS = 0.1, 0.9, 1e-4, 0.5, 1e-8
CHUNK = 16384  # KS_NORM_CHUNK: elements one stage-1 block owns
STEPS = 3


def _specs():
    """(kind, shape): 224 two-dimensional tensors around the vector and
    chunk edges (more than two launches of 110), then the special ones."""
    specs = [("plain", (1, n)) for n in (1, 3, 7, 8, CHUNK - 1, CHUNK,
                                         CHUNK + 1, 3 * CHUNK + 5)] * 28
    specs.append(("channels_last", (128, 64, 3, 3)))
    specs.append(("offset", (1, CHUNK + 9)))  # p, g, v 4 bytes off 16
    specs.append(("none", (1, 1000)))         # never has a gradient
    specs.append(("zero", (1, 1000)))         # all-zero gradient: trust 1
    specs.append(("vector", (1000,)))         # 1-D: LARS excludes it
    return specs


def _offset_view(t):  # t's values, 4 bytes off 16-byte alignment
    buf = torch.empty(t.numel() + 8, device="cuda")
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


@pytest.fixture(scope="module")
def case():
    gen = torch.Generator(device="cuda").manual_seed(31)
    specs = _specs()
    init, grads = [], [[] for _ in range(STEPS + 1)]
    for kind, shape in specs:
        p = torch.randn(shape, device="cuda", generator=gen)
        if kind == "channels_last":
            p = p.contiguous(memory_format=torch.channels_last)
        init.append(p)
        for gs in grads:
            g = torch.randn(shape, device="cuda", generator=gen)
            if kind == "channels_last":
                g = g.contiguous(memory_format=torch.channels_last)
            gs.append(None if kind == "none" else
                      torch.zeros_like(g) if kind == "zero" else g)
    return {"specs": specs, "init": init, "grads": grads,
            "norm0": _norm64(grads[0])[0].item()}


def _norm64(tensors):
    each = torch.stack([torch.linalg.vector_norm(
        (torch.zeros(1, device="cuda") if t is None else t).double())
        for t in tensors])
    return torch.linalg.vector_norm(each), each


def _reference(case, grad_sets, max_norm, lars):
    """The issue's formulas in f64: (p, v, last global norm)."""
    ps = [p.double() for p in case["init"]]
    vs = [torch.zeros_like(p) for p in ps]
    for grads in grad_sets:
        norm = _norm64(grads)[0]
        c = torch.clamp(max_norm / (norm + 1e-6), max=1.0) if max_norm else 1.0
        for p, v, g in zip(ps, vs, grads):
            if g is None:
                continue
            cg = c * g.double()
            if lars and p.ndim > 1:
                wn = torch.linalg.vector_norm(p)
                gn = torch.linalg.vector_norm(cg)
                trust = lars * wn / (gn + WD * wn + EPS) \
                    if wn > 0 and gn > 0 else 1.0
                v.mul_(MU).add_(trust * (WD * p + cg))
            else:
                v.mul_(MU).add_(cg + WD * p)
            p.sub_(LR * v)
    return ps, vs, norm


def _optimizer(case, **kw):
    """FusedSGD over fresh copies; "offset": p and v misaligned too."""
    ps = [(_offset_view(p) if kind == "offset" else p.clone())
          .requires_grad_() for (kind, _), p in zip(case["specs"],
                                                    case["init"])]
    opt = ops.FusedSGD(ps, lr=LR, momentum=MU, weight_decay=WD, **kw)
    for i, (kind, _) in enumerate(case["specs"]):
        if kind == "offset":
            opt.momenta[i] = _offset_view(opt.momenta[i])
    return opt


def _step(opt, case, grads, none_as_zero=False):
    for p, (kind, _), g in zip(opt.params, case["specs"], grads):
        if g is None:
            p.grad = torch.zeros_like(p) if none_as_zero else None
        else:
            p.grad = _offset_view(g) if kind == "offset" else g.clone()
    opt.step()


def _assert_same_bits(case, a, b):
    for spec, p, q, v, w in zip(case["specs"], a.params, b.params,
                                a.momenta, b.momenta):
        assert torch.equal(p, q) and torch.equal(v, w), spec


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_norm_matches_f64(case, dtype):
    ts = [None if g is None else
          _offset_view(g) if kind == "offset" and dtype == torch.float32
          else g.to(dtype) for (kind, _), g in zip(case["specs"],
                                                   case["grads"][0])]
    total, each = ops.grad_norm(ts, per_tensor=True)
    want_total, want_each = _norm64(ts)
    torch.testing.assert_close(total.double(), want_total, rtol=1e-5, atol=0)
    torch.testing.assert_close(each.double(), want_each, rtol=1e-5, atol=0)
    again, each2 = ops.grad_norm(ts, per_tensor=True)
    assert torch.equal(total, again) and torch.equal(each, each2)


@pytest.mark.parametrize("clip,lars", [(True, None), (False, ETA),
                                       (True, ETA)])
def test_step_matches_f64(case, clip, lars):
    max_norm = 0.5 * case["norm0"] if clip else None
    opt = _optimizer(case, max_grad_norm=max_norm, lars=lars)
    for s in range(STEPS):
        _step(opt, case, case["grads"][s])
    ref_p, ref_v, ref_norm = _reference(case, case["grads"][:STEPS],
                                        max_norm, lars)
    torch.testing.assert_close(opt.grad_norm.double(), ref_norm, rtol=1e-5,
                               atol=0)
    assert int(opt.nonfinite_steps) == 0
    for i, (kind, _) in enumerate(case["specs"]):
        for got, want in ((opt.params[i], ref_p[i]),
                          (opt.momenta[i], ref_v[i])):
            torch.testing.assert_close(got.detach().double(), want,
                                       rtol=1e-5, atol=1e-6, msg=lambda m:
                                       f"{case['specs'][i]}: {m}")
        if kind == "none":  # no gradient: untouched
            assert torch.equal(opt.params[i], case["init"][i])


def test_idle_clip_is_the_plain_step(case):
    idle, plain = _optimizer(case, max_grad_norm=1e30), _optimizer(case)
    for s in range(STEPS):
        _step(idle, case, case["grads"][s])
        _step(plain, case, case["grads"][s])
    _assert_same_bits(case, idle, plain)


def test_graph_replay_recomputes_the_norm(case):
    """Replays read norm, coefficient and trust ratios on the device."""
    opts = [_optimizer(case, max_grad_norm=0.5 * case["norm0"], lars=ETA,
                       graph_mode=mode) for mode in ("auto", "off")]
    for opt in opts:
        _step(opt, case, case["grads"][0], none_as_zero=True)
        assert (opt._step_graph is not None) == (opt is opts[0])
        opt.step()
        for p, g in zip(opt.params, case["grads"][1]):
            if g is not None:
                p.grad.copy_(10.0 * g)
        opt.step()
    _assert_same_bits(case, *opts)
    assert torch.equal(opts[0].grad_norm, opts[1].grad_norm)
    assert opts[0].grad_norm.item() > 5.0 * case["norm0"]


def test_nonfinite_step_is_skipped(case):
    opt = _optimizer(case, max_grad_norm=1.0, lars=ETA)
    _step(opt, case, case["grads"][0])
    before = [(p.detach().clone(), v.clone())
              for p, v in zip(opt.params, opt.momenta)]
    bad = list(case["grads"][1])
    bad[5] = bad[5].clone()
    bad[5].view(-1)[2] = float("inf")
    _step(opt, case, bad)
    for (p0, v0), p, v in zip(before, opt.params, opt.momenta):
        assert torch.equal(p, p0) and torch.equal(v, v0)
    assert int(opt.nonfinite_steps) == 1
    # the next step is that of an optimizer that never saw the inf
    ref = _optimizer(case, max_grad_norm=1.0, lars=ETA)
    for g in (case["grads"][0], case["grads"][2]):
        _step(ref, case, g)
    _step(opt, case, case["grads"][2])
    _assert_same_bits(case, opt, ref)
    assert int(opt.nonfinite_steps) == 1


@pytest.fixture(scope="module")
def world_of_one(tmp_path_factory):
    import torch.distributed as dist
    store = tmp_path_factory.mktemp("pg") / "store"
    dist.init_process_group(
        "gloo", init_method=f"file://{store}", rank=0, world_size=1,
        timeout=datetime.timedelta(seconds=60))
    try:
        yield dist.group.WORLD
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_grouped_is_the_ungrouped_step(case, world_of_one, dtype):
    kw = dict(max_grad_norm=0.5 * case["norm0"], lars=ETA)
    grouped = _optimizer(case, process_group=world_of_one, grad_dtype=dtype,
                         **kw)
    plain = _optimizer(case, **kw)
    for s in range(STEPS):
        _step(grouped, case, case["grads"][s])
        # what the bucket holds: zeros for None, values rounded
        _step(plain, case, [None if g is None else g.to(dtype).float()
                            for g in case["grads"][s]], none_as_zero=True)
    _assert_same_bits(case, grouped, plain)
    assert torch.equal(grouped.grad_norm, plain.grad_norm)


def test_launch_count_for_161_tensors():
    """ResNet50's 161 tensors: 2 + 1 + 2 kernels, 2 with neither flag."""
    from torch.profiler import ProfilerActivity, profile
    for kw, most in ((dict(max_grad_norm=1.0, lars=ETA), 5), ({}, 2)):
        ps = [torch.randn(1, 64 + i, device="cuda").requires_grad_()
              for i in range(161)]
        opt = ops.FusedSGD(ps, lr=LR, momentum=MU, weight_decay=WD,
                           graph_mode="off", **kw)
        for p in ps:
            p.grad = torch.randn_like(p)
        opt.step()  # code objects loaded outside the profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU,
                                 ProfilerActivity.CUDA]) as prof:
            opt.step()
            torch.cuda.synchronize()
        kernels = [e.name for e in prof.events()
                   if e.device_type == torch.autograd.DeviceType.CUDA]
        assert 1 <= len(kernels) <= most, kernels
        assert kw or all("sgd_mom_multi_f32" in k for k in kernels), kernels
