"""Per-shape microbench: fused ks_ops NHWC bf16 max-pool vs stock
F.max_pool2d, forward and forward+backward, on the ResNet stem pool at
batch 256 and VGG16's five pools at batch 64. Event-timed after warm-up;
the paths run alternately and the round is repeated so the spread is
visible. Prints one JSON line per shape (--out also writes them to a
file).

Two times per path, both between device events around `iters`
back-to-back calls:
  *_ms       GPU time: a calibrated ops.burn() kernel is queued first, so
             the host has every launch enqueued before the first event
             fires (what the op costs inside a training step, where the
             host runs ahead of the GPU);
  *_call_ms  no priming: the rate of the bare call. At the small shapes
             this is the host's launch path, not the kernels.
`iters` is sized per shape so that a sample spans about --window-ms.

`need_mb` is what the algorithm has to move, from the shape alone:
  forward           x read + y write + 1-byte argmax write
  forward+backward  the above + dy read + argmax read + dx write
and `*_gbs` is that figure over the median GPU time (for the stock path
it is the same useful bytes, not what that path really moves)."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = [  # (name, (N, C, H, W), (k, s, p))
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
    import torch.nn.functional as F
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
        assert ops.max_pool_supported(x, k, s, p)
        xg = x.clone().requires_grad_()
        oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        dy = torch.randn(n, c, oh, ow, device="cuda").to(torch.bfloat16)\
            .contiguous(memory_format=torch.channels_last)

        def stock_fwd():
            with torch.no_grad():
                F.max_pool2d(x, k, s, p)

        def fused_fwd():
            with torch.no_grad():
                ops.max_pool_nhwc(x, k, s, p)

        def stock_fb():
            F.max_pool2d(xg, k, s, p).backward(dy)
            xg.grad = None

        def fused_fb():
            ops.max_pool_nhwc(xg, k, s, p).backward(dy)
            xg.grad = None

        fns = {"stock_fwd": stock_fwd, "fused_fwd": fused_fwd,
               "stock_fb": stock_fb, "fused_fb": fused_fb}
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
        need_fwd = 2 * n_in + 2 * n_out + n_out
        need_fb = need_fwd + 2 * n_out + n_out + 2 * n_in
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
            r[key + "_call_min_ms"] = round(min(call[key]), 4)
            r[key + "_call_max_ms"] = round(max(call[key]), 4)
            r[key + "_iters"] = iters[key]
        r["fwd_speedup"] = round(r["stock_fwd_ms"] / r["fused_fwd_ms"], 2)
        r["fb_speedup"] = round(r["stock_fb_ms"] / r["fused_fb_ms"], 2)
        r["fwd_call_speedup"] = round(
            r["stock_fwd_call_ms"] / r["fused_fwd_call_ms"], 2)
        r["fb_call_speedup"] = round(
            r["stock_fb_call_ms"] / r["fused_fb_call_ms"], 2)
        line = json.dumps(r)
        print(line, flush=True)
        lines.append(line)
        del x, xg, dy
        torch.cuda.empty_cache()

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)),
                    exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
