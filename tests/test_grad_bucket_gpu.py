"""hip/grad_bucket.hip and the grouped ops.FusedSGD on the GPU.

  - pack against the torch expression (g * f32(scale)).to(dtype), bit for
    bit, both bucket dtypes, scales 1, 1/2 and 1/3, over every size and
    layout at which the kernel takes another path;
  - unpack round trips;
  - sgd_momentum_multi_bf16g_ against sgd_momentum_multi_ fed the upcast
    views;
  - FusedSGD(process_group=<group of one>) against FusedSGD();
  - two ranks sharing the GPU over gloo against a local reference;
  - a two-rank gang on the fused path end to end (launch_gang).

Run as a script (`test_grad_bucket_gpu.py rank <r> <world> <store>
<dtype>`) this file is one rank of test_two_ranks_one_gpu."""
import datetime
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import pytest  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from kubeshare_amd import ops  # noqa: E402

CHUNK = 8192         # KS_GB_CHUNK: elements one pack block owns
MAX_TENSORS = 128    # KS_GB_MAX_TENSORS: tensors per pack launch
SGD_MAX_TENSORS = 110
LR, MU, WD = 0.1, 0.9, 1e-4
STEPS = 3
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
SCALES = [1.0, 0.5, 1.0 / 3.0]


def _f32(bits):
    return torch.tensor([bits], dtype=torch.int32).view(torch.float32).item()


# NaN (one whose payload sits in the low mantissa bits only), +-inf,
# -0.0, a denormal, bf16 ties: 1 + 2^-8 is halfway between 0x3F80 and
# 0x3F81 (to even: down), 1 + 3 * 2^-8 between 0x3F81 and 0x3F82 (up),
# and their negatives
SPECIALS = [float("nan"), _f32(0x7F800001), float("inf"), float("-inf"),
            -0.0, 1e-40, _f32(0x3F808000), _f32(0x3F818000),
            _f32(0xBF808000 - (1 << 32)), _f32(0xBF818000 - (1 << 32))]


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _offset_view(t):
    """t's values in a view that starts 4 bytes into a larger buffer."""
    buf = torch.empty(t.numel() + 8, device="cuda")
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _specs():
    """(kind, shape): the sizes around the vector and chunk edges, the
    layouts, and 300 small tensors (more than two launches' worth)."""
    specs = [("plain", (n,)) for n in
             (1, 3, 7, 8, 9, 1000, 4097, CHUNK, 2 * CHUNK + 5)]
    specs.append(("channels_last", (128, 64, 3, 3)))
    specs.append(("none", (1000,)))
    # a contiguous gradient for a channels-last parameter
    specs.append(("restride", (16, 8, 3, 3)))
    # source 4 bytes off 16-byte alignment: scalar path, across a chunk
    specs.append(("offset", (CHUNK + 9,)))
    specs.append(("offset", (8,)))
    specs += [("plain", (1 + i % 13,)) for i in range(300)]
    return specs


def _param(kind, shape):
    p = torch.zeros(shape, device="cuda")
    if kind in ("channels_last", "restride"):
        p = p.contiguous(memory_format=torch.channels_last)
    return p


def _values(specs, seed):
    """One seeded f32 tensor per spec, in the parameter's layout, with
    the special values rotated through its first elements."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    sp = torch.tensor(SPECIALS, device="cuda")
    out = []
    for i, (kind, shape) in enumerate(specs):
        t = torch.randn(shape, device="cuda", generator=g)
        flat = t.view(-1)
        k = min(flat.numel(), len(SPECIALS))
        flat[:k] = sp.roll(-i)[:k]
        if kind == "channels_last":
            t = t.contiguous(memory_format=torch.channels_last)
        out.append(t)
    return out


def _sources(specs, vals):
    srcs = []
    for (kind, _), t in zip(specs, vals):
        if kind == "none":
            srcs.append(None)
        elif kind == "offset":
            srcs.append(_offset_view(t))
        else:
            srcs.append(t)  # "restride": NCHW-contiguous as generated
    return srcs


def _padding_mask(b):
    pad = torch.ones(b.flat.numel(), dtype=torch.bool, device="cuda")
    for p, off in zip(b.params, b.offsets):
        pad[off:off + p.numel()] = False
    return pad


@pytest.fixture(scope="module")
def case():
    specs = _specs()
    vals = _values(specs, 3)
    torch.cuda.synchronize()
    return {"specs": specs, "vals": vals,
            "params": [_param(k, s) for k, s in specs]}


# ---------------------------------------------------------------- pack
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_pack_is_bit_exact(case, dtype_name, scale):
    dtype = DTYPES[dtype_name]
    specs, vals = case["specs"], case["vals"]
    b = ops.GradBucket(case["params"], dtype)
    assert all(off % 8 == 0 for off in b.offsets)
    pad = _padding_mask(b)
    b.flat.fill_(7.0)  # stale segment contents must not survive
    b.flat[pad] = 0.0
    srcs = _sources(specs, vals)
    b.pack(srcs, scale)
    s32 = torch.tensor(scale, dtype=torch.float32).item()
    for (kind, shape), v, t in zip(specs, b.views, vals):
        if kind == "none":
            want = torch.zeros(shape, device="cuda", dtype=dtype)
        else:
            want = (t * s32).to(dtype)
        assert v.shape == want.shape
        assert torch.equal(_bits(v), _bits(want)), (kind, shape)
    assert torch.count_nonzero(b.flat[pad]) == 0
    assert int(pad.sum()) > 0


def test_pack_launch_count(case):
    """More than MAX_TENSORS tensors take ceil(n / MAX_TENSORS)
    launches; a None entry still owns a segment to zero."""
    b = ops.GradBucket(case["params"], torch.float32)
    n = len(case["specs"])
    assert n > 2 * MAX_TENSORS
    launches = ops._load().grad_pack_multi(
        _sources(case["specs"], case["vals"]), b.flat, b.offsets, 1.0,
        b.views)
    assert launches == -(-n // MAX_TENSORS)


def test_pack_rejects_what_would_leave_the_buffer(case):
    ext = ops._load()
    b = ops.GradBucket(case["params"][:3], torch.float32)
    srcs = case["vals"][:3]
    with pytest.raises(RuntimeError):
        ext.grad_pack_multi(srcs, b.flat, [0, 8, b.flat.numel() - 1], 1.0,
                            b.views)
    with pytest.raises(RuntimeError):
        ext.grad_pack_multi(srcs, b.flat, [0, 8, -8], 1.0, b.views)
    with pytest.raises(RuntimeError):  # wrong shape for its segment
        ext.grad_pack_multi([srcs[1], srcs[0], srcs[2]], b.flat, b.offsets,
                            1.0, b.views)
    with pytest.raises(RuntimeError):  # CPU source for a CUDA bucket
        ext.grad_pack_multi([s.cpu() for s in srcs], b.flat, b.offsets,
                            1.0, b.views)
    torch.cuda.synchronize()


# -------------------------------------------------------------- unpack
@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_unpack_round_trip(case, dtype_name):
    dtype = DTYPES[dtype_name]
    specs, vals = case["specs"], case["vals"]
    b = ops.GradBucket(case["params"], dtype)
    srcs = _sources(specs, vals)
    b.pack(srcs)
    outs = []
    for (kind, _), p in zip(specs, case["params"]):
        o = torch.full_like(p, 3.0)
        outs.append(_offset_view(o) if kind == "offset" else o)
    b.unpack(outs)
    for (kind, shape), o, t in zip(specs, outs, vals):
        if kind == "none":
            want = torch.zeros(shape, device="cuda")
        elif dtype == torch.float32:
            want = t * 1.0  # what pack's one multiply makes of a NaN
        else:
            want = t.bfloat16().float()
        assert torch.equal(_bits(o), _bits(want)), (kind, shape)


# ------------------------------------------- SGD from a bf16 bucket
def _sgd_specs():
    specs = [("plain", (n,)) for n in (1, 3, 7, 8, 1000, 4097)] * 20
    specs.append(("channels_last", (128, 64, 3, 3)))
    specs.append(("plain", (3 * 4096 + 5,)))
    specs.append(("offset", (4096 + 9,)))  # p and v on the scalar path
    return specs


def _sgd_inputs(seed):
    specs = _sgd_specs()
    g = torch.Generator(device="cuda").manual_seed(seed)
    init, grads = [], [[] for _ in range(STEPS)]
    for kind, shape in specs:
        p = torch.randn(shape, device="cuda", generator=g)
        if kind == "channels_last":
            p = p.contiguous(memory_format=torch.channels_last)
        init.append(p)
        for s in range(STEPS):
            gr = torch.randn(shape, device="cuda", generator=g)
            if kind == "channels_last":
                gr = gr.contiguous(memory_format=torch.channels_last)
            grads[s].append(gr)
    return specs, init, grads


def _clone_params(specs, init):
    return [(_offset_view(p) if kind == "offset" else p.clone())
            for (kind, _), p in zip(specs, init)]


def test_sgd_from_bf16_bucket_matches_f32_kernel():
    ext = ops._load()
    specs, init, grads = _sgd_inputs(21)
    assert len(specs) > SGD_MAX_TENSORS
    pa, pb = _clone_params(specs, init), _clone_params(specs, init)
    va = [_offset_view(torch.zeros_like(p)) if k == "offset"
          else torch.zeros_like(p) for (k, _), p in zip(specs, pa)]
    vb = [_offset_view(torch.zeros_like(p)) if k == "offset"
          else torch.zeros_like(p) for (k, _), p in zip(specs, pb)]
    b = ops.GradBucket(pa, torch.bfloat16)
    for s in range(STEPS):
        b.pack(grads[s], 0.5)
        na = ext.sgd_momentum_multi_bf16g_(pa, b.views, va, LR, MU, WD)
        up = [v.float() for v in b.views]
        assert all(u.stride() == p.stride() for u, p in zip(up, pb))
        nb = ext.sgd_momentum_multi_(pb, up, vb, LR, MU, WD)
        assert na == nb == 2
    torch.cuda.synchronize()
    for spec, x, y, vx, vy in zip(specs, pa, pb, va, vb):
        assert torch.equal(_bits(x), _bits(y)), spec
        assert torch.equal(_bits(vx), _bits(vy)), spec
    # f32 gradients are refused, not reinterpreted
    with pytest.raises(RuntimeError):
        ext.sgd_momentum_multi_bf16g_(pa, grads[0], va, LR, MU, WD)


# --------------------------------------- FusedSGD with a group of one
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


@pytest.mark.parametrize("with_none", [False, True])
def test_fused_sgd_group_of_one(world_of_one, with_none):
    """A world of one averages nothing: the grouped optimizer must be
    the ungrouped one bit for bit; a None gradient counts as zeros."""
    specs, init, grads = _sgd_inputs(22)
    pa = [p.detach().requires_grad_() for p in _clone_params(specs, init)]
    pb = [p.detach().requires_grad_() for p in _clone_params(specs, init)]
    grouped = ops.FusedSGD(pa, lr=LR, momentum=MU, weight_decay=WD,
                           process_group=world_of_one)
    plain = ops.FusedSGD(pb, lr=LR, momentum=MU, weight_decay=WD)
    assert plain._bucket is None and grouped._bucket is not None
    for s in range(STEPS):
        grouped.zero_grad()
        plain.zero_grad()
        for i, (a, b_, gr) in enumerate(zip(pa, pb, grads[s])):
            if with_none and i % 7 == 3:
                a.grad = None
                b_.grad = torch.zeros_like(b_)
            else:
                a.grad = gr.clone()
                b_.grad = gr.clone()
        grouped.step()
        plain.step()
    torch.cuda.synchronize()
    for spec, a, b_, va, vb in zip(specs, pa, pb, grouped.momenta,
                                   plain.momenta):
        assert torch.equal(_bits(a.data), _bits(b_.data)), spec
        assert torch.equal(_bits(va), _bits(vb)), spec


def test_default_group_and_argument_checks(world_of_one):
    p = torch.randn(9, device="cuda").requires_grad_()
    opt = ops.FusedSGD([p], lr=LR, process_group=True,
                       grad_dtype=torch.bfloat16)
    assert opt._bucket.flat.dtype == torch.bfloat16
    with pytest.raises(ValueError):
        ops.FusedSGD([p], lr=LR, grad_dtype=torch.bfloat16)


# ------------------------------------------- two ranks on one GPU
RANK_SHAPES = [(5,), (16, 8, 3, 3), (9,), (1000,), (CHUNK + 3,)]
RANK_CL = 1
RANK_NONE = (1, 1, 2)  # (step, rank, index) whose gradient is None


def _rank_grads(step, rank):
    g = torch.Generator(device="cuda").manual_seed(100 + 10 * step + rank)
    out = []
    for i, s in enumerate(RANK_SHAPES):
        t = torch.randn(s, device="cuda", generator=g)
        if i == RANK_CL:
            t = t.contiguous(memory_format=torch.channels_last)
        out.append(None if (step, rank, i) == RANK_NONE else t)
    return out


def _rank_params():
    g = torch.Generator(device="cuda").manual_seed(7)
    ps = []
    for i, s in enumerate(RANK_SHAPES):
        t = torch.randn(s, device="cuda", generator=g)
        if i == RANK_CL:
            t = t.contiguous(memory_format=torch.channels_last)
        ps.append(t.requires_grad_())
    return ps


def _rank_main(rank, world, store, dtype_name):
    import torch.distributed as dist
    dtype = DTYPES[dtype_name]
    assert world == 2
    dist.init_process_group(
        "gloo", init_method="file://" + store, rank=rank, world_size=world,
        timeout=datetime.timedelta(seconds=60))
    try:
        ps, ref = _rank_params(), _rank_params()
        opt = ops.FusedSGD(ps, lr=LR, momentum=MU, weight_decay=WD,
                           process_group=True, grad_dtype=dtype)
        ref_opt = ops.FusedSGD(ref, lr=LR, momentum=MU, weight_decay=WD)
        for step in range(STEPS):
            both = [_rank_grads(step, r) for r in range(world)]
            opt.zero_grad()
            ref_opt.zero_grad()
            for p, g in zip(ps, both[rank]):
                p.grad = g
            for i, p in enumerate(ref):
                # each term scaled in f32 and rounded to the wire dtype,
                # then added in it
                terms = [torch.zeros_like(p, dtype=dtype) if gs[i] is None
                         else (gs[i] * 0.5).to(dtype) for gs in both]
                p.grad = (terms[0] + terms[1]).float()
            opt.step()
            ref_opt.step()
        torch.cuda.synchronize()
        for i, (p, q, v, w) in enumerate(zip(ps, ref, opt.momenta,
                                             ref_opt.momenta)):
            assert torch.equal(_bits(p.data), _bits(q.data)), (i, dtype_name)
            assert torch.equal(_bits(v), _bits(w)), (i, dtype_name)
        cs = sum(int(_bits(p.data).sum(dtype=torch.int64)) for p in ps)
        print(f"CHECKSUM {cs}", flush=True)
    finally:
        dist.destroy_process_group()


def _run_ranks(argv_tail, world, store, timeout):
    """One plain subprocess per rank of this file's script mode; every
    one is waited for with a hard limit and killed past it."""
    procs = [subprocess.Popen(
        [sys.executable, os.path.abspath(__file__), "rank", str(r),
         str(world), store] + argv_tail,
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
        cwd=REPO) for r in range(world)]
    outs = []
    try:
        for p in procs:
            try:
                outs.append(p.communicate(timeout=timeout)[0])
            except subprocess.TimeoutExpired:
                p.kill()
                outs.append("TIMEOUT\n" + p.communicate()[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    return [(p.returncode, o) for p, o in zip(procs, outs)]


@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_two_ranks_one_gpu(tmp_path, dtype_name):
    res = _run_ranks([dtype_name], 2, str(tmp_path / "store"), timeout=180)
    sums = []
    for r, (code, out) in enumerate(res):
        assert code == 0, (r, code, out)
        lines = [ln for ln in out.splitlines() if ln.startswith("CHECKSUM ")]
        assert len(lines) == 1, (r, out)
        sums.append(lines[0])
    assert sums[0] == sums[1], sums


# ------------------------------------------------------ gang end to end
@pytest.mark.parametrize("grad_dtype,port", [("f32", 29581), ("bf16", 29583)])
def test_fused_gang_two_ranks_one_gpu(native_bins, grad_dtype, port):
    """Two token-gated ranks sharing the GPU train resnet18 on the fused
    path; each rank raises if the replicas' parameter checksums differ
    after the run, which launch_gang reports as not ok. (The limit
    allows for MIOpen compiling kernels on a cold cache.)"""
    from kubeshare_amd.parallel import launch_gang
    ok, stats = launch_gang(ranks=2, share_gpu=True, fused=True,
                            model="resnet18", batch=8, image_size=64,
                            steps=3, timeout=240, grad_dtype=grad_dtype,
                            master_port=port)
    assert ok, f"fused gang failed or diverged; stats={stats}"


if __name__ == "__main__":
    assert sys.argv[1] == "rank"
    _rank_main(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5])
