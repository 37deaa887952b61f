#!/usr/bin/env python3
"""bench.py — the BASELINE.json headline benchmark.

Metric: aggregate images/sec + quota-error % for N co-located pods at
gpu_request=0.5 per MI355X. Per GPU (= per rank) this stands up the full
production isolation chain — gpu-schd, one pod-mgr per pod, and TWO pod
processes with LD_PRELOAD=libhiphook.so — each training the flagship
model (ResNet50, bf16 autocast, channels-last, synthetic data,
random-init weights) for exactly --steps full training steps.

Launch (driver contract):
  python bench.py --gpus 1 --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
      --master-addr 127.0.0.1 bench.py --gpus N --steps K --warmup W

`value` is the WHOLE-JOB aggregate images/s over all pods on all N GPUs;
`ms_per_step` is the max-over-ranks time for the K steps of the
co-located pair. Quota enforcement error (server-side, from gpu-schd's
sliding-window accounting) is reported in config.quota_error_pct.

A plain run sets up, warms up, times the K steps and prints the result
line. `--dump-outputs DIR` additionally has every pod write what its
last timed step computed (see bench_worker.dump_outputs). Inputs and
initial weights are seeded per pod name, and with this option each pod
rewinds its weights, BN buffers and momenta to that seeded state right
before the last timed step: training from random init amplifies the
ulp-level run-to-run noise of MIOpen's atomic weight-gradient kernels
to percents within a few steps, whereas one step from fixed state is
reproducible (conv weights, which those kernels update, stay out of
the dump), so two builds can be compared file for file (and
config.per_pod_loss is then the initial-state loss, about ln 1000).
`--full` is where secondary measurements that need runs of their own
belong; there are none today.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)


def ensure_native():
    from kubeshare_amd.isolation.local import NATIVE_DIR
    needed = ["gpu-schd", "pod-mgr", "libhiphook.so"]
    if not all(os.path.exists(os.path.join(NATIVE_DIR, n)) for n in needed):
        subprocess.run(["make", "-C", NATIVE_DIR], check=True,
                       capture_output=True)


def _quota_error(st0: dict, st1: dict) -> dict:
    """Per-pod |achieved GPU-time share - entitled share| in % over the
    timed region, from gpu-schd's cumulative per-pod counters (server-
    side: a pod cannot fake it)."""
    used = {}
    for pod, v in st1.get("pods", {}).items():
        before = st0.get("pods", {}).get(pod, {}).get("total_used_ms", 0.0)
        used[pod] = max(0.0, v["total_used_ms"] - before)
    total = sum(used.values())
    if total <= 0:
        return {}
    reqs = {p: st1["pods"][p]["request"] for p in used}
    total_req = sum(reqs.values()) or 1.0
    return {p: abs(used[p] / total - reqs[p] / total_req) * 100.0
            for p in used}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--model", default="resnet50")
    ap.add_argument("--batch", type=int, default=256,
                    help="per-pod batch size")
    ap.add_argument("--image-size", type=int, default=224)
    ap.add_argument("--pods-per-gpu", type=int, default=2)
    ap.add_argument("--request", type=float, default=0.5)
    ap.add_argument("--limit", type=float, default=1.0)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--quota-ms", type=float, default=None,
                    help="override gpu-schd base quota (-q); default "
                         "keeps the reference's 300 ms")
    ap.add_argument("--device", default=None,
                    help="override (cpu for plumbing tests)")
    ap.add_argument("--use-ops", default="auto")
    # HIP multi-tensor SGD measured ~4.7% faster end-to-end than
    # torch.optim.SGD on MI355X (same semantics, numerics-tested)
    ap.add_argument("--fused-sgd", action=argparse.BooleanOptionalAction,
                    default=True)
    # the tuned MIOpen db shipped in kubeshare_amd/ops/miopen_udb already
    # names the fastest solver for every flagship conv shape: measured
    # 31.5 ms/step solo either way, but the exhaustive find costs ~60 s
    # per pod at the first warmup step (~110 s for a co-located pair)
    ap.add_argument("--miopen-find", action=argparse.BooleanOptionalAction,
                    default=False,
                    help="benchmark every MIOpen solver per conv shape "
                         "during warmup; use it for a model or batch size "
                         "the shipped tuned db does not cover")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what each pod's "
                         "last timed step computed (loss, logits, a fixed "
                         "seeded sample of the updated BN/fc parameters) as "
                         "float32 DIR/pod<rank>-<i>.<name>.npy; that step "
                         "starts from the seeded initial state")
    ap.add_argument("--full", action="store_true",
                    help="also run the benchmark's secondary measurements; "
                         "there are none today (the quota error comes from "
                         "the timed run itself), so this changes nothing")
    args = ap.parse_args()

    import torch

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    distributed = world > 1

    on_gpu = torch.cuda.is_available() and args.device != "cpu"

    dist = None
    if distributed:
        import torch.distributed as dist_mod
        dist = dist_mod
        backend = "nccl" if on_gpu else "gloo"
        if on_gpu:
            torch.cuda.set_device(local_rank)
        dist.init_process_group(backend=backend)

    ensure_native()
    from kubeshare_amd.isolation.local import LocalGPUShare

    share = LocalGPUShare(gpu_index=local_rank,
                          full_memory=(torch.cuda.get_device_properties(
                              local_rank).total_memory if on_gpu
                              else 288 * 1024**3))
    if args.quota_ms:
        share.base_quota_ms = args.quota_ms
    share.start()

    workers = []
    try:
        for i in range(args.pods_per_gpu):
            pod_name = f"bench/pod{local_rank}-{i}"
            h = share.add_pod(pod_name, request=args.request,
                              limit=args.limit)
            env = h.env(gpu_index=local_rank)
            if not on_gpu:
                env.pop("KUBESHARE_REQUIRE_HOOK", None)
            # the pod sees exactly one GPU (ROCR_VISIBLE_DEVICES) -> cuda:0
            wdev = "cuda:0" if on_gpu else "cpu"
            cmd = [sys.executable, "-m", "kubeshare_amd.bench_worker",
                   "--model", args.model, "--batch", str(args.batch),
                   "--image-size", str(args.image_size),
                   "--steps", str(args.steps), "--warmup", str(args.warmup),
                   "--device", wdev, "--dtype",
                   "bf16" if args.dtype == "bf16" else "fp32",
                   "--use-ops", args.use_ops] \
                  + (["--fused-sgd"] if args.fused_sgd else []) \
                  + ["--miopen-find" if args.miopen_find
                     else "--no-miopen-find"]
            if args.dump_outputs:
                cmd += ["--dump-outputs", os.path.abspath(args.dump_outputs),
                        "--dump-name", f"pod{local_rank}-{i}"]
            env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
            p = subprocess.Popen(cmd, env=env, cwd=REPO,
                                 stdin=subprocess.PIPE,
                                 stdout=subprocess.PIPE, text=True,
                                 bufsize=1)
            workers.append((pod_name, p))

        # wait for warmup on every pod of this rank
        for name, p in workers:
            line = p.stdout.readline().strip()
            if line != "READY":
                raise RuntimeError(f"{name}: expected READY, got {line!r} "
                                   f"(exit={p.poll()})")

        # ---- timed region: barrier + device sync on both sides ----
        if dist:
            dist.barrier()
        if on_gpu:
            torch.cuda.synchronize()
        st0 = share.stats()  # cumulative per-pod GPU ms before the region
        t0 = time.perf_counter()
        for _, p in workers:
            p.stdin.write("GO\n")
            p.stdin.flush()
        results = []
        for name, p in workers:
            line = p.stdout.readline().strip()
            if not line.startswith("DONE"):
                raise RuntimeError(f"{name}: expected DONE, got {line!r}")
            _, elapsed_s, images, loss = line.split()
            results.append((float(elapsed_s), int(images), float(loss)))
        if on_gpu:
            torch.cuda.synchronize()
        t1 = time.perf_counter()
        if dist:
            dist.barrier()
        elapsed = t1 - t0

        # let the hook watchdogs RET the final leases so the cumulative
        # counters include the tail of the timed region
        time.sleep(0.4)
        stats = share.stats()
        quota_err = _quota_error(st0, stats)

        if args.dump_outputs:
            for name, p in workers:
                line = p.stdout.readline().strip()
                if line != "DUMPED":
                    raise RuntimeError(f"{name}: expected DUMPED, got "
                                       f"{line!r} (exit={p.poll()})")
    finally:
        for _, p in workers:
            if p.poll() is None:
                p.kill()
        share.stop()

    rank_images = sum(r[1] for r in results)

    if dist:
        t = torch.tensor([elapsed], dtype=torch.float64)
        n = torch.tensor([float(rank_images)], dtype=torch.float64)
        if on_gpu:
            t, n = t.cuda(), n.cuda()
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dist.all_reduce(n, op=dist.ReduceOp.SUM)
        max_elapsed = float(t.item())
        total_images = float(n.item())
    else:
        max_elapsed = elapsed
        total_images = float(rank_images)

    if rank == 0:
        pods_total = args.pods_per_gpu * world
        mean_qerr = (sum(quota_err.values()) / len(quota_err)
                     if quota_err else None)
        out = {
            "metric": "aggregate images/sec, co-located shared-GPU pods",
            "value": round(total_images / max_elapsed, 2),
            "unit": "images/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(max_elapsed / args.steps * 1000.0, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,  # reference publishes no numbers
            "dtype": args.dtype,
            "data": "synthetic",
            "config": {
                "model": args.model,
                "global_batch": args.batch * pods_total,
                "image_size": args.image_size,
                "parallelism": f"{pods_total} pods @ request="
                               f"{args.request}, {args.pods_per_gpu}/GPU",
                "pods_per_gpu": args.pods_per_gpu,
                "gpu_request": args.request,
                "gpu_limit": args.limit,
                "miopen_find": args.miopen_find,
                "quota_error_pct": round(mean_qerr, 3)
                                    if mean_qerr is not None else None,
                "quota_error_per_pod": {k: round(v, 3)
                                        for k, v in quota_err.items()},
                "sched_window_ms": stats.get("window_ms"),
                "lease_accounting": ("sampled-busy"
                                     if stats.get("sampler")
                                     else "wall/RET"),
                "grants_per_pod": {p: v.get("grants")
                                   for p, v in stats["pods"].items()},
                "per_pod_loss": [r[2] for r in results],
            },
        }
        print(json.dumps(out), flush=True)

    if dist:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
