"""Cost of the gradient bucket on ResNet50's parameter list.

Times, with device events around ITERS back-to-back calls after a
warm-up, what a grouped ops.FusedSGD step adds to an ungrouped one on
the device: GradBucket.pack (f32 and bf16 bucket), and for context the
multi-tensor SGD reading the bucket's views in either dtype against the
SGD reading the gradients themselves. Prints one JSON line per
measurement (microseconds per call, bytes moved, GB/s).

    python tools/grad_bucket_bench.py [--iters 200] [--model resnet50]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def timed(fn, iters, warmup=20):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1000.0 / iters  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--model", default="resnet50")
    args = ap.parse_args()

    import torch

    from kubeshare_amd import ops
    from kubeshare_amd.models import build_model

    assert torch.cuda.is_available(), "grad_bucket_bench needs a GPU"
    ext = ops._load()
    model = build_model(args.model).cuda().to(
        memory_format=torch.channels_last)
    params = [p.data for p in model.parameters()]
    grads = [torch.randn_like(p) for p in params]
    momenta = [torch.zeros_like(p) for p in params]
    n = sum(p.numel() for p in params)
    world = 2

    def report(name, us, nbytes):
        print(json.dumps({
            "bench": name, "model": args.model, "tensors": len(params),
            "elements": n, "us_per_call": round(us, 2),
            "bytes": nbytes, "gb_per_s": round(nbytes / us / 1e3, 1),
            "iters": args.iters}), flush=True)

    for name, dtype, width in (("f32", torch.float32, 4),
                               ("bf16", torch.bfloat16, 2)):
        bucket = ops.GradBucket(params, dtype)
        us = timed(lambda: bucket.pack(grads, 1.0 / world), args.iters)
        report(f"pack_{name}", us, n * (4 + width))
        sgd = ext.sgd_momentum_multi_ if dtype == torch.float32 \
            else ext.sgd_momentum_multi_bf16g_
        us = timed(lambda: sgd(params, bucket.views, momenta, 0.0, 0.9, 0.0),
                   args.iters)
        report(f"sgd_from_{name}_bucket", us, n * (16 + width))
    us = timed(lambda: ext.sgd_momentum_multi_(params, grads, momenta, 0.0,
                                               0.9, 0.0), args.iters)
    report("sgd_from_gradients", us, n * 20)


if __name__ == "__main__":
    main()
