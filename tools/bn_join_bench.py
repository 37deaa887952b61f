"""Per-shape microbench: the fused downsample join (ops.bn_join,
hip/bn_join.hip) vs the composition
ops.bn_relu(x, bn, res=ops.bn_relu(x_d, bn_d, relu=False), fork=True) it
replaces, training-mode forward (under no_grad) and forward+backward
with two upstream gradients (the forked join of the real network), on
ResNet50's four downsample shapes at batch 256. Event-timed after
warm-up; the paths run alternately in the same session and the round is
repeated so the spread is visible. Prints one JSON line per shape (--out
also writes them to a file; the committed record is
profiles/bn_join_bench.json).

Timing is tools/bn_pool_bench.py's: `*_ms` is GPU time between device
events around `iters` back-to-back calls with a calibrated ops.burn()
queued first; `*_call_ms` is the same without priming.

`need_*_mb` is what the fused algorithm has to move, from the shape
alone (n elements per tensor, 2 bytes each, mask n/8 bytes):
  forward           x and x_d read twice (statistics, apply) + y write
                    (+ mask write when a gradient is required)
  forward+backward  the above + stats: x, x_d, dy, dy2, mask read, dym
                    write; apply: x, x_d, dym read, dx, dx_d write
and `*_gbs` is that figure over the median GPU time (for the composition
it is the same useful bytes, not what that path really moves).

KUBESHARE_BN_MASK=0 in the environment times both paths with the
y-reading backward kernels instead."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = [  # (name, (N, C, H, W) of the join)
    ("layer1.0", (256, 256, 56, 56)),
    ("layer2.0", (256, 512, 28, 28)),
    ("layer3.0", (256, 1024, 14, 14)),
    ("layer4.0", (256, 2048, 7, 7)),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the lines here")
    args = ap.parse_args()

    import torch
    from kubeshare_amd import ops

    sync = torch.cuda.synchronize

    def timed(fn, iters, prime_ms=0.0):
        """(event ms, host enqueue ms) per call over `iters` calls."""
        ev0 = torch.cuda.Event(enable_timing=True)
        ev1 = torch.cuda.Event(enable_timing=True)
        if prime_ms:
            ops.burn(prime_ms)
        t0 = time.perf_counter()
        ev0.record()
        for _ in range(iters):
            fn()
        ev1.record()
        host = (time.perf_counter() - t0) * 1000
        sync()
        return ev0.elapsed_time(ev1) / iters, host / iters

    def rand(shape):
        return torch.randn(shape, device="cuda").to(torch.bfloat16)\
            .contiguous(memory_format=torch.channels_last)

    lines = []
    for name, shape in SHAPES:
        c = shape[1]
        x, x_d, g1, g2 = rand(shape), rand(shape), rand(shape), rand(shape)
        xg, xdg = x.clone().requires_grad_(), x_d.clone().requires_grad_()
        bn = torch.nn.BatchNorm2d(c).cuda()
        bn_d = torch.nn.BatchNorm2d(c).cuda()
        with torch.no_grad():
            for m in (bn, bn_d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.5, 0.5)
        assert ops.bn_join_enabled() and ops.bn_join_supported(x, x_d)

        def comp(a, b):
            return ops.bn_relu(a, bn, res=ops.bn_relu(b, bn_d, relu=False),
                               fork=True)

        def fused(a, b):
            return ops.bn_join(a, bn, b, bn_d, fork=True)

        def drop_grads():
            xg.grad = None
            xdg.grad = None
            for m in (bn, bn_d):
                m.weight.grad = None
                m.bias.grad = None

        def comp_fwd():
            with torch.no_grad():
                comp(x, x_d)

        def fused_fwd():
            with torch.no_grad():
                fused(x, x_d)

        def comp_fb():
            torch.autograd.backward(comp(xg, xdg), [g1, g2])
            drop_grads()

        def fused_fb():
            torch.autograd.backward(fused(xg, xdg), [g1, g2])
            drop_grads()

        probe = fused(xg, xdg)  # a silent fall-back would time the wrong thing
        assert "BNJoinFn" in probe[0].grad_fn.name()
        del probe
        fns = {"comp_fwd": comp_fwd, "fused_fwd": fused_fwd,
               "comp_fb": comp_fb, "fused_fb": fused_fb}
        iters, host_ms = {}, {}
        for key, fn in fns.items():
            for _ in range(args.warmup):
                fn()
            sync()
            t, hms = timed(fn, 20)
            iters[key] = max(20, min(2000, int(args.window_ms / t) + 1))
            host_ms[key] = hms
        gpu = {key: [] for key in fns}
        call = {key: [] for key in fns}
        for _ in range(args.repeats):   # alternate the paths
            for key, fn in fns.items():
                t, hms = timed(fn, iters[key])
                call[key].append(t)
                host_ms[key] = max(host_ms[key], hms)
            for key, fn in fns.items():
                # burn long enough for the host to enqueue every call
                prime = 1.5 * host_ms[key] * iters[key] + 1.0
                gpu[key].append(timed(fn, iters[key], prime)[0])

        n = x.numel()
        mask = n // 8 if ops.bn_mask_enabled() else 2 * n
        need_fwd = 2 * n * 5
        need_fb = need_fwd + (mask if ops.bn_mask_enabled() else 0) \
            + 2 * n * 5 + mask + 2 * n * 5
        r = {"name": name, "shape": list(shape),
             "mask": ops.bn_mask_enabled(),
             "need_fwd_mb": round(need_fwd / 1e6, 1),
             "need_fb_mb": round(need_fb / 1e6, 1)}
        for key in fns:
            med = statistics.median(gpu[key])
            r[key + "_ms"] = round(med, 4)
            r[key + "_min_ms"] = round(min(gpu[key]), 4)
            r[key + "_max_ms"] = round(max(gpu[key]), 4)
            need = need_fwd if key.endswith("fwd") else need_fb
            r[key + "_gbs"] = round(need / med / 1e6, 1)
            r[key + "_call_ms"] = round(statistics.median(call[key]), 4)
            r[key + "_iters"] = iters[key]
        r["fwd_speedup"] = round(r["comp_fwd_ms"] / r["fused_fwd_ms"], 2)
        r["fb_speedup"] = round(r["comp_fb_ms"] / r["fused_fb_ms"], 2)
        line = json.dumps(r)
        print(line, flush=True)
        lines.append(line)
        del x, x_d, g1, g2, xg, xdg, bn, bn_d
        torch.cuda.empty_cache()

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)),
                    exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
