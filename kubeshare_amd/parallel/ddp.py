"""DDP gang under the isolation chain.

`ddp_worker` is the per-rank training loop (RCCL on GPU, gloo on CPU);
`launch_gang` stands up the full sharing stack — gpu-schd, pod-mgr per
rank, LD_PRELOAD hook — and runs N ranks either one-per-GPU (the
supported gang config) or all on ONE GPU (the hazardous config:
two ranks sharing a device, where gating a collective would deadlock;
kept alive by the RCCL exemption + gang co-granting + the `group`
field of the per-UUID config file). With fused=True the ranks train on
the fused path (ops.fuse_model + ops.FusedSGD averaging one flat
gradient bucket per step) instead of stock modules under
DistributedDataParallel.

Used by tools/ddp_gang.py (CLI) and tests/test_gpu_isolation.py (the
RCCL-under-sharing hardware proof).
"""
from __future__ import annotations

import os
import subprocess
import sys
import time

_REPO = os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))


def _step(model, opt, x, y, autocast):
    import torch
    opt.zero_grad(set_to_none=True)
    if autocast:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = torch.nn.functional.cross_entropy(model(x), y)
    else:
        loss = torch.nn.functional.cross_entropy(model(x), y)
    loss.backward()
    opt.step()
    return loss


def _grad_dtype(grad_dtype):
    """"f32" / "bf16" (the CLI's spelling) or a torch dtype."""
    import torch
    if isinstance(grad_dtype, torch.dtype):
        return grad_dtype
    try:
        return {"f32": torch.float32, "bf16": torch.bfloat16}[grad_dtype]
    except KeyError:
        raise ValueError(f"grad_dtype {grad_dtype!r}: 'f32' or 'bf16'")


def _check_replicas(model):
    """Raise unless every rank holds the same parameter bits: each rank
    packs its parameters into a bucket and sums the buffer's 32-bit
    words into a 64-bit checksum; the checksums are all-gathered and
    compared. A diverged gang thereby exits non-zero."""
    import torch
    import torch.distributed as dist

    from .. import ops

    params = [p.data for p in model.parameters()]
    bucket = ops.GradBucket(params, torch.float32)
    bucket.pack(params)
    mine = bucket.flat.view(torch.int32).sum(dtype=torch.int64).reshape(1)
    every = [torch.zeros_like(mine) for _ in range(dist.get_world_size())]
    dist.all_gather(every, mine)
    sums = [int(c.item()) for c in every]
    if len(set(sums)) != 1:
        raise RuntimeError(f"gang replicas diverged: rank {dist.get_rank()} "
                           f"sees parameter checksums {sums}")
    return sums[0]


def ddp_worker(model_name: str = "resnet18", batch: int = 32,
               image_size: int = 224, steps: int = 10,
               warmup: int = 3, fused: bool = False,
               grad_dtype="f32") -> float:
    """One DDP rank: init from the torchrun/env contract, train
    `steps` timed steps, return ms/step (rank 0 also prints a
    DDP_RESULT line).

    fused=True trains on the fused path instead of the stock modules
    under DistributedDataParallel: ops.fuse_model, channels-last, bf16
    autocast, NO DDP wrapper; ops.broadcast_parameters once, then
    ops.FusedSGD(process_group=True, grad_dtype=...) averages the
    gradients with one all-reduce of a flat bucket per step ("f32" or
    "bf16" on the wire). After the timed steps the ranks compare a
    checksum of their parameters and raise if they differ. Needs a
    GPU."""
    import torch
    import torch.distributed as dist

    from ..models import build_model

    on_gpu = torch.cuda.is_available()
    if fused and not on_gpu:
        raise RuntimeError("ddp_worker(fused=True) needs a GPU: the fused "
                           "path has no CPU kernels")
    # RCCL refuses two ranks on one device ("Duplicate GPU detected" —
    # same restriction as NCCL; the reference's own gang workloads only
    # ever put one NCCL rank per GPU, test/distribute/*). For the
    # shared-GPU gang config the launcher therefore selects gloo
    # gradients over GPU compute; whole-GPU gangs use RCCL.
    backend = os.environ.get("KUBESHARE_DDP_BACKEND") or \
        ("nccl" if on_gpu else "gloo")
    dist.init_process_group(backend)
    dev = "cuda" if on_gpu else "cpu"
    if on_gpu:
        torch.cuda.set_device(0)  # ROCR_VISIBLE_DEVICES narrows the view
    if fused:
        from .. import ops
        from ..utils.tuning import apply_miopen_tuning
        apply_miopen_tuning()  # before the first conv
        model = ops.fuse_model(build_model(model_name)).to(dev).to(
            memory_format=torch.channels_last)
        ops.broadcast_parameters(model, src=0)
        opt = ops.FusedSGD(model.parameters(), lr=0.01, momentum=0.9,
                           process_group=True,
                           grad_dtype=_grad_dtype(grad_dtype))
    else:
        model = build_model(model_name).to(dev)
        if on_gpu:
            model = model.to(memory_format=torch.channels_last)
        model = torch.nn.parallel.DistributedDataParallel(model)
        opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9)
    x = torch.randn(batch, 3, image_size, image_size, device=dev)
    if on_gpu:
        x = x.contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 1000, (batch,), device=dev)
    for _ in range(warmup):
        _step(model, opt, x, y, autocast=on_gpu)
    if on_gpu:
        torch.cuda.synchronize()
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        _step(model, opt, x, y, autocast=on_gpu)
    if on_gpu:
        torch.cuda.synchronize()
    dist.barrier()
    dt = (time.perf_counter() - t0) / steps * 1000
    if fused:
        _check_replicas(model)
    if dist.get_rank() == 0:
        print(f"DDP_RESULT ms_per_step={dt:.2f}", flush=True)
    dist.destroy_process_group()
    return dt


def launch_gang(ranks: int = 2, share_gpu: bool = False, steps: int = 10,
                model: str = "resnet18", batch: int = 32,
                image_size: int = 224, timeout: float = 300.0,
                master_port: int = 29571, fused: bool = False,
                grad_dtype: str = "f32"):
    """Run a DDP gang under the full isolation chain. Returns
    (all_ok, per_gpu_stats) where per_gpu_stats is each
    LocalGPUShare's final gpu-schd STATS dict (server-side quota
    accounting, keyed by pod). fused / grad_dtype ("f32" or "bf16")
    are ddp_worker's: the gang trains on the fused path, and a gang
    whose replicas diverged reports not ok."""
    if grad_dtype not in ("f32", "bf16"):
        raise ValueError(f"grad_dtype {grad_dtype!r}: 'f32' or 'bf16'")
    from ..isolation.local import LocalGPUShare

    shares, procs = [], []
    stats = []
    try:
        if share_gpu:
            shares.append(LocalGPUShare(gpu_index=0).start())
        else:
            for i in range(ranks):
                shares.append(LocalGPUShare(gpu_index=i).start())
        handles = []
        for r in range(ranks):
            share = shares[0] if share_gpu else shares[r]
            handles.append(share.add_pod(
                f"gang/rank{r}",
                request=(1.0 / ranks) if share_gpu else 1.0,
                limit=1.0))
        # the `group` field in the per-UUID config makes gpu-schd
        # co-grant the gang when ranks share a GPU — set BEFORE any
        # worker can REQ
        for share in shares:
            _mark_gang(share)
        time.sleep(0.2)  # let inotify reload land
        for r in range(ranks):
            gpu = 0 if share_gpu else r
            env = handles[r].env(gpu_index=gpu)
            env.update({
                "RANK": str(r), "LOCAL_RANK": str(r),
                "WORLD_SIZE": str(ranks),
                "MASTER_ADDR": "127.0.0.1",
                "MASTER_PORT": str(master_port),
                "PYTHONPATH": _REPO + os.pathsep +
                env.get("PYTHONPATH", ""),
            })
            if share_gpu:
                env["KUBESHARE_DDP_BACKEND"] = "gloo"  # see ddp_worker
            procs.append(subprocess.Popen(
                [sys.executable, "-c",
                 "from kubeshare_amd.parallel.ddp import ddp_worker; "
                 f"ddp_worker({model!r}, {batch}, {image_size}, {steps}, "
                 f"fused={bool(fused)}, grad_dtype={grad_dtype!r})"],
                env=env, cwd=_REPO))
        deadline = time.time() + timeout
        for p in procs:
            p.wait(timeout=max(1.0, deadline - time.time()))
        for share in shares:
            stats.append(share.stats())
        return all(p.returncode == 0 for p in procs), stats
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for s in shares:
            s.stop()


def _mark_gang(share):
    """Rewrite the share's per-UUID config with the gang group set
    (config-file 5th field, native/common/protocol.hpp)."""
    from ..configdaemon import files as F
    quotas = [F.PodQuota(h.name, h.limit, h.request, h.memory, group="gang")
              for h in share.pods.values()]
    F.write_gpu_config(share.config_dir, share.uuid, quotas)
