"""Multi-tensor SGD (sgd_mom_multi_f32_kernel via ops.FusedSGD) against
the per-tensor `sgd_momentum_` kernel (bit-exact reference: both share
one update function) and torch.optim.SGD (rtol 1e-5 / atol 1e-6)."""
import math
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

LR, MU, WD = 0.1, 0.9, 1e-4
CHUNK = 4096        # KS_SGD_CHUNK: elements one block owns
MAX_TENSORS = 110   # KS_SGD_MAX_TENSORS: triples per launch
STEPS = 3


def _specs():
    """(kind, shape) of every parameter: ~200 tiny tensors around the
    float4 / chunk edges, then the special layouts."""
    specs = [("plain", (n,)) for n in (1, 3, 7, 8, 1000, 4097)] * 33
    specs.append(("plain", (3, 3, 17)))
    # more than two whole chunks plus a ragged, non-float4 tail
    specs.append(("plain", (3 * CHUNK + 5,)))
    specs.append(("channels_last", (128, 64, 3, 3)))
    # p, g and v all 4 bytes off 16-byte alignment (scalar path), across
    # a chunk edge; then only g off
    specs.append(("offset_all", (CHUNK + 9,)))
    specs.append(("offset_all", (8,)))
    specs.append(("offset_grad", (1000,)))
    return specs


def _offset_view(t):
    """t's values in a view that starts 4 bytes into a larger buffer."""
    buf = torch.empty(t.numel() + 8, device="cuda")
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


@pytest.fixture(scope="module")
def case():
    """Initial parameters, per-step gradients (None for every 7th
    parameter) and the two references after STEPS steps; computed once,
    read-only for the tests."""
    g = torch.Generator(device="cuda").manual_seed(11)
    specs = _specs()
    init, grads = [], [[] for _ in range(STEPS)]
    for i, (kind, shape) in enumerate(specs):
        p = torch.randn(shape, device="cuda", generator=g)
        if kind == "channels_last":
            p = p.contiguous(memory_format=torch.channels_last)
        init.append(p)
        for s in range(STEPS):
            if i % 7 == 3:
                grads[s].append(None)
                continue
            gr = torch.randn(shape, device="cuda", generator=g)
            if kind == "channels_last":
                gr = gr.contiguous(memory_format=torch.channels_last)
            grads[s].append(gr)

    # reference 1: the per-tensor kernel on aligned clones
    ext = ops._load()
    ref_p = [p.clone() for p in init]
    ref_v = [torch.zeros_like(p) for p in init]
    for s in range(STEPS):
        idx = [i for i, gr in enumerate(grads[s]) if gr is not None]
        ext.sgd_momentum_([ref_p[i] for i in idx],
                          [grads[s][i] for i in idx],
                          [ref_v[i] for i in idx], LR, MU, WD)

    # reference 2: torch.optim.SGD
    tp = [p.clone().requires_grad_() for p in init]
    topt = torch.optim.SGD(tp, lr=LR, momentum=MU, weight_decay=WD)
    for s in range(STEPS):
        topt.zero_grad(set_to_none=True)
        for p, gr in zip(tp, grads[s]):
            p.grad = None if gr is None else gr.clone()
        topt.step()
    torch.cuda.synchronize()
    return {"specs": specs, "init": init, "grads": grads,
            "ref_p": ref_p, "ref_v": ref_v, "torch_p": tp}


def _make_params(case):
    ps = []
    for (kind, _), p0 in zip(case["specs"], case["init"]):
        p = _offset_view(p0) if kind == "offset_all" else p0.clone()
        ps.append(p.detach().requires_grad_())
    return ps


def _fresh_grad(kind, gr):
    if gr is None:
        return None
    if kind in ("offset_all", "offset_grad"):
        return _offset_view(gr)
    return gr.clone()


def test_multi_matches_per_tensor_and_torch(case):
    ps = _make_params(case)
    opt = ops.FusedSGD(ps, lr=LR, momentum=MU, weight_decay=WD)
    for i, (kind, _) in enumerate(case["specs"]):
        if kind == "offset_all":
            opt.momenta[i] = _offset_view(opt.momenta[i])
    for s in range(STEPS):
        opt.zero_grad()
        assert all(p.grad is None for p in ps)
        # fresh gradient tensors every step, as a backward pass that
        # found no .grad to accumulate into leaves them
        for p, (kind, _), gr in zip(ps, case["specs"], case["grads"][s]):
            p.grad = _fresh_grad(kind, gr)
        opt.step()
    torch.cuda.synchronize()
    for i, (p, v) in enumerate(zip(ps, opt.momenta)):
        assert torch.equal(p, case["ref_p"][i]), case["specs"][i]
        assert torch.equal(v, case["ref_v"][i]), case["specs"][i]
        torch.testing.assert_close(p, case["torch_p"][i],
                                   rtol=1e-5, atol=1e-6)


def test_zero_grad_sets_none():
    ps = [torch.randn(5, device="cuda").requires_grad_() for _ in range(4)]
    opt = ops.FusedSGD(ps, lr=LR, momentum=MU, weight_decay=WD)
    for _ in range(3):  # also once the step graph exists
        for p in ps:
            p.grad = torch.randn_like(p)
        opt.step()
        opt.zero_grad()
        assert all(p.grad is None for p in ps)
    opt.step()  # nothing to do: every gradient is None
    torch.cuda.synchronize()


def test_gradient_strides_are_matched():
    """A contiguous gradient for a channels-last parameter (rare path)
    is re-strided, not misread as flat storage."""
    torch.manual_seed(5)
    w = torch.randn(16, 8, 3, 3, device="cuda").contiguous(
        memory_format=torch.channels_last)
    g = torch.randn(16, 8, 3, 3, device="cuda")  # NCHW-contiguous
    ref = w.clone().requires_grad_()
    ref.grad = g.clone()
    torch.optim.SGD([ref], lr=LR, momentum=MU, weight_decay=WD).step()
    p = w.clone().requires_grad_()
    p.grad = g
    ops.FusedSGD([p], lr=LR, momentum=MU, weight_decay=WD).step()
    torch.testing.assert_close(p, ref, rtol=1e-5, atol=1e-6)


def test_launch_count_for_161_tensors():
    """ResNet50 has 161 parameter tensors: one step is
    ceil(161 / 110) = 2 kernels, counted on the device."""
    from torch.profiler import ProfilerActivity, profile
    n = 161
    designed = math.ceil(n / MAX_TENSORS)
    ps = [torch.randn(64 + i, device="cuda").requires_grad_()
          for i in range(n)]
    opt = ops.FusedSGD(ps, lr=LR, momentum=MU, weight_decay=WD,
                       graph_mode="off")
    for p in ps:
        p.grad = torch.randn_like(p)
    opt.step()  # code object loaded outside the profile
    ext = ops._load()
    assert ext.sgd_momentum_multi_(
        [p.data for p in ps], [p.grad for p in ps], opt.momenta,
        LR, MU, WD) == designed
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU,
                             ProfilerActivity.CUDA]) as prof:
        opt.step()
        torch.cuda.synchronize()
    kernels = [e.name for e in prof.events()
               if e.device_type == torch.autograd.DeviceType.CUDA]
    assert 1 <= len(kernels) <= designed, kernels
    assert all("sgd_mom_multi" in k for k in kernels), kernels


def test_step_replays_inside_cuda_graph(case):
    """The multi-tensor launch captured by torch.cuda.graph replays the
    update (pointers and block table are baked into the node)."""
    ext = ops._load()
    ps = [p.clone() for p in case["init"]]
    vs = [torch.zeros_like(p) for p in ps]
    # one persistent gradient set: step 0's, zeros where it has None
    gs = [torch.zeros_like(p) if gr is None else gr.clone()
          for p, gr in zip(ps, case["grads"][0])]
    ref_p = [p.clone() for p in ps]
    ref_v = [torch.zeros_like(p) for p in ps]
    for _ in range(STEPS):
        ext.sgd_momentum_(ref_p, gs, ref_v, LR, MU, WD)

    ext.sgd_momentum_multi_(ps, gs, vs, LR, MU, WD)  # eager step 1
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ext.sgd_momentum_multi_(ps, gs, vs, LR, MU, WD)
    for _ in range(STEPS - 1):
        graph.replay()
    torch.cuda.synchronize()
    for p, v, rp, rv in zip(ps, vs, ref_p, ref_v):
        assert torch.equal(p, rp)
        assert torch.equal(v, rv)


def test_fused_sgd_graph_replays_only_on_same_pointers(case):
    """Persistent gradients: steps 2-3 replay the captured step. A fresh
    gradient set afterwards must launch eagerly and still be exact."""
    ps = [p.clone().requires_grad_() for p in case["init"][:40]]
    gs = [torch.randn_like(p) for p in ps]
    ext = ops._load()
    ref_p = [p.detach().clone() for p in ps]
    ref_v = [torch.zeros_like(p) for p in ref_p]
    for _ in range(STEPS + 1):
        ext.sgd_momentum_(ref_p, gs, ref_v, LR, MU, WD)
    opt = ops.FusedSGD(ps, lr=LR, momentum=MU, weight_decay=WD)
    for p, g in zip(ps, gs):
        p.grad = g.clone()
    for _ in range(STEPS):
        opt.step()
    assert opt._step_graph is not None
    opt.zero_grad()
    for p, g in zip(ps, gs):
        p.grad = g.clone()
    opt.step()
    torch.cuda.synchronize()
    for p, v, rp, rv in zip(ps, opt.momenta, ref_p, ref_v):
        assert torch.equal(p, rp)
        assert torch.equal(v, rv)
