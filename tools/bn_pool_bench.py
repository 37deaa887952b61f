"""Per-shape microbench: fused BN+ReLU+max-pool (ops.bn_relu_pool,
hip/bn_pool.hip) vs the composition ops.max_pool_nhwc(ops.bn_relu(x, bn))
it replaces, training-mode forward (under no_grad) and forward+backward,
on the ResNet stem at batch 256 and VGG16's five pre-pool shapes at
batch 64. Event-timed after warm-up; the paths run alternately in the
same session and the round is repeated so the spread is visible. Prints
one JSON line per shape (--out also writes them to a file; the committed
record is profiles/bn_pool_bench.json).

Timing is tools/pool_bench.py's: `*_ms` is GPU time between device
events around `iters` back-to-back calls with a calibrated ops.burn()
queued first, so the host has every launch enqueued before the first
event fires; `*_call_ms` is the same without priming (the rate of the
bare call). `iters` is sized per shape so that a sample spans about
--window-ms.

`need_*_mb` is what the fused algorithm has to move, from the shape
alone (n_in, n_out elements before / after the pool):
  forward           x read twice (statistics, apply) + y write
  forward+backward  the above + 1-byte codes write, and per backward
                    kernel x, dy and the codes read; + dx write
and `*_gbs` is that figure over the median GPU time (for the composition
it is the same useful bytes, not what that path really moves)."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = [  # (name, (N, C, H, W) before the pool, (k, s, p))
    ("resnet_stem", (256, 64, 112, 112), (3, 2, 1)),
    ("vgg16_pool1", (64, 64, 224, 224), (2, 2, 0)),
    ("vgg16_pool2", (64, 128, 112, 112), (2, 2, 0)),
    ("vgg16_pool3", (64, 256, 56, 56), (2, 2, 0)),
    ("vgg16_pool4", (64, 512, 28, 28), (2, 2, 0)),
    ("vgg16_pool5", (64, 512, 14, 14), (2, 2, 0)),
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

    lines = []
    for name, (n, c, h, w), (k, s, p) in SHAPES:
        x = torch.randn(n, c, h, w, device="cuda").to(torch.bfloat16)\
            .contiguous(memory_format=torch.channels_last)
        assert ops.bn_relu_pool_supported(x, k, s, p)
        xg = x.clone().requires_grad_()
        bn = torch.nn.BatchNorm2d(c).cuda()
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.5, 0.5)
        oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        dy = torch.randn(n, c, oh, ow, device="cuda").to(torch.bfloat16)\
            .contiguous(memory_format=torch.channels_last)

        def comp(t):
            return ops.max_pool_nhwc(ops.bn_relu(t, bn), k, s, p)

        def fused(t):
            return ops.bn_relu_pool(t, bn, k, s, p)

        def drop_grads():
            xg.grad = None
            bn.weight.grad = None
            bn.bias.grad = None

        def comp_fwd():
            with torch.no_grad():
                comp(x)

        def fused_fwd():
            with torch.no_grad():
                fused(x)

        def comp_fb():
            comp(xg).backward(dy)
            drop_grads()

        def fused_fb():
            fused(xg).backward(dy)
            drop_grads()

        probe = fused(xg)  # a silent fall-back would time the wrong thing
        assert "BNReLUMaxPoolNHWCFn" in probe.grad_fn.name()
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

        n_in, n_out = x.numel(), dy.numel()
        need_fwd = 4 * n_in + 2 * n_out
        need_fb = need_fwd + n_out + 2 * (2 * n_in + 3 * n_out) + 2 * n_in
        r = {"name": name, "shape": [n, c, h, w], "ksp": [k, s, p],
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
        del x, xg, dy, bn
        torch.cuda.empty_cache()

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)),
                    exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
