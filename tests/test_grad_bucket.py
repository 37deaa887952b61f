"""ops.GradBucket on CPU tensors: the flat layout (offsets, padding,
views), pack / unpack as the torch expressions they are defined by, and
a two-rank gloo all-reduce of the bucket against the sum torch computes.
The kernels behind the same interface are tests/test_grad_bucket_gpu.py.

Run as a script (`test_grad_bucket.py rank <r> <world> <store> <dtype>`)
this file is one gloo rank of test_two_ranks_all_reduce."""
import datetime
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import pytest  # noqa: E402

torch = pytest.importorskip("torch")

from kubeshare_amd import ops  # noqa: E402

SHAPES = [(5,), (16, 8, 3, 3), (9,), (1000,), (3, 3, 17), (8,)]
CL = 1          # index of the channels-last parameter
NONE_AT = (1, 2)  # (rank, index) whose gradient is None
SCALE = 0.5
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def _params():
    ps = [torch.zeros(s) for s in SHAPES]
    ps[CL] = ps[CL].contiguous(memory_format=torch.channels_last)
    return ps


def _rank_grads(rank):
    """Rank `rank`'s gradients, derivable by every rank."""
    g = torch.Generator().manual_seed(100 + rank)
    out = []
    for i, s in enumerate(SHAPES):
        t = torch.randn(s, generator=g)
        if i == CL:
            t = t.contiguous(memory_format=torch.channels_last)
        out.append(None if (rank, i) == NONE_AT else t)
    return out


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ------------------------------------------------------------- layout
@pytest.mark.parametrize("dtype", list(DTYPES.values()))
def test_layout(dtype):
    ps = _params()
    b = ops.GradBucket(ps, dtype)
    assert b.flat.dtype == dtype and b.flat.dim() == 1
    assert len(b.offsets) == len(b.views) == len(ps)
    end = 0
    for p, off, v in zip(ps, b.offsets, b.views):
        assert off % 8 == 0
        assert off >= end  # segments do not overlap
        end = off + p.numel()
        assert v.size() == p.size() and v.stride() == p.stride()
        assert v.storage_offset() == off
        assert v.dtype == dtype
    assert b.flat.numel() >= end and b.flat.numel() % 8 == 0
    assert b.views[CL].is_contiguous(memory_format=torch.channels_last)
    assert b.views[CL].stride() == (72, 1, 24, 8)
    assert torch.count_nonzero(b.flat) == 0


def test_default_dtype_is_f32():
    assert ops.GradBucket(_params()).flat.dtype == torch.float32


def test_non_dense_parameter_raises():
    with pytest.raises(ValueError):
        ops.GradBucket([torch.zeros(8, 8)[:, ::2]])
    with pytest.raises(ValueError):
        ops.GradBucket([torch.zeros(4, 1).expand(4, 3)])
    with pytest.raises(ValueError):
        ops.GradBucket(_params(), torch.float16)
    # a permuted dense tensor is fine
    ops.GradBucket([torch.zeros(4, 6).t()])


def _padding_mask(b):
    pad = torch.ones(b.flat.numel(), dtype=torch.bool)
    for p, off in zip(b.params, b.offsets):
        pad[off:off + p.numel()] = False
    return pad


@pytest.mark.parametrize("dtype", list(DTYPES.values()))
@pytest.mark.parametrize("scale", [1.0, 0.5, 1.0 / 3.0])
def test_pack_is_the_torch_expression(dtype, scale):
    ps = _params()
    b = ops.GradBucket(ps, dtype)
    b.flat.fill_(7.0)  # stale segment contents must not survive
    pad = _padding_mask(b)
    b.flat[pad] = 0.0
    gs = _rank_grads(1)
    # a contiguous gradient for the channels-last parameter
    gs[CL] = gs[CL].contiguous()
    b.pack(gs, scale)
    s32 = torch.tensor(scale, dtype=torch.float32)
    for v, g, p in zip(b.views, gs, ps):
        want = torch.zeros_like(p) if g is None else g * s32
        assert torch.equal(_bits(v), _bits(want.to(dtype))), p.shape
    assert torch.count_nonzero(b.flat[pad]) == 0
    assert pad.sum() > 0


@pytest.mark.parametrize("dtype", list(DTYPES.values()))
def test_unpack_round_trips(dtype):
    ps = _params()
    b = ops.GradBucket(ps, dtype)
    xs = _rank_grads(0)
    b.pack(xs)
    out = [torch.full_like(p, 3.0) for p in ps]
    out[2] = None  # skipped
    b.unpack(out)
    for i, (x, o) in enumerate(zip(xs, out)):
        if o is None:
            continue
        assert o.stride() == ps[i].stride()
        assert torch.equal(_bits(o), _bits(x.to(dtype).float()))
    with pytest.raises(ValueError):
        b.unpack(out[:-1])
    out[CL] = out[CL].contiguous()
    with pytest.raises(ValueError):
        b.unpack(out)


# ---------------------------------------------------------- two ranks
def _rank_main(rank, world, store, dtype_name):
    import torch.distributed as dist
    dtype = DTYPES[dtype_name]
    dist.init_process_group(
        "gloo", init_method="file://" + store, rank=rank, world_size=world,
        timeout=datetime.timedelta(seconds=60))
    try:
        b = ops.GradBucket(_params(), dtype)
        b.pack(_rank_grads(rank), SCALE)
        b.all_reduce()
        per_rank = [_rank_grads(r) for r in range(world)]
        for i, v in enumerate(b.views):
            # each term rounded to the bucket dtype, then added in it
            terms = [torch.zeros(SHAPES[i], dtype=dtype) if gs[i] is None
                     else (gs[i] * SCALE).to(dtype) for gs in per_rank]
            want = terms[0] + terms[1]
            assert want.dtype == dtype
            assert torch.equal(_bits(v), _bits(want)), (i, dtype_name)
        assert torch.count_nonzero(b.flat[_padding_mask(b)]) == 0
        print(f"RANK_OK {rank}", flush=True)
    finally:
        dist.destroy_process_group()


def _run_ranks(argv_tail, world, store, timeout):
    """One subprocess per rank of this file's script mode; every one is
    waited for with a hard limit and killed past it."""
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
def test_two_ranks_all_reduce(tmp_path, dtype_name):
    res = _run_ranks([dtype_name], 2, str(tmp_path / "store"), timeout=120)
    for r, (code, out) in enumerate(res):
        assert code == 0 and f"RANK_OK {r}" in out, (r, code, out)


if __name__ == "__main__":
    assert sys.argv[1] == "rank"
    _rank_main(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5])
