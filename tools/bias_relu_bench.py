"""Per-shape microbench: fused bias+ReLU(+max-pool) (ops.bias_relu /
ops.bias_relu_pool, hip/bias_relu.hip) vs the stock elementwise sequence
it replaces, on the 13 conv-output shapes of VGG16 at batch 64, forward
(under no_grad) and forward+backward including the bias gradient.
Event-timed after warm-up; the paths run alternately in the same session
and the round is repeated so the spread is visible. Prints one JSON line
per shape (--out also writes them to a file; the committed record is
profiles/bias_relu_bench.json).

Stock sequence: the add of the bf16 bias, the ReLU and, at the five pool
sites, ops.max_pool_nhwc; backward, what autograd runs for them
(threshold_backward, the bias-gradient sum, the pool backward). The
training step applies the add and the ReLU in place on the conv output;
here they are out of place (x + b, then relu), because an in-place pair
would consume the input of the next iteration. The traffic is the same:
each of the two kernels reads one tensor and writes one.

Timing is tools/pool_bench.py's: `*_ms` is GPU time between device
events around `iters` back-to-back calls with a calibrated ops.burn()
queued first, so the host has every launch enqueued before the first
event fires; `*_call_ms` is the same without priming (the rate of the
bare call). `iters` is sized per shape so that a sample spans about
--window-ms.

`need_*_mb` is what the fused algorithm has to move, from the shape
alone (n_in, n_out elements before / after the pool; n_out = n_in
without a pool):
  forward           x read + y write
  forward+backward  the above + dy and y read, dx write; with a pool
                    also the 1-byte codes written and read
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

BATCH = 64
SHAPES = [  # (name, (C, H, W) of the conv output, pool after it?)
    ("conv1_1", (64, 224, 224), False),
    ("conv1_2", (64, 224, 224), True),
    ("conv2_1", (128, 112, 112), False),
    ("conv2_2", (128, 112, 112), True),
    ("conv3_1", (256, 56, 56), False),
    ("conv3_2", (256, 56, 56), False),
    ("conv3_3", (256, 56, 56), True),
    ("conv4_1", (512, 28, 28), False),
    ("conv4_2", (512, 28, 28), False),
    ("conv4_3", (512, 28, 28), True),
    ("conv5_1", (512, 14, 14), False),
    ("conv5_2", (512, 14, 14), False),
    ("conv5_3", (512, 14, 14), True),
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
    for name, (c, h, w), pool in SHAPES:
        n = BATCH
        x = torch.randn(n, c, h, w, device="cuda").to(torch.bfloat16)\
            .contiguous(memory_format=torch.channels_last)
        if pool:
            assert ops.bias_relu_pool_supported(x, 2, 2, 0)
        else:
            assert ops.bias_relu_supported(x)
        xg = x.clone().requires_grad_()
        b32 = (torch.rand(c, device="cuda") - 0.5).requires_grad_()
        b16 = b32.detach().to(torch.bfloat16).requires_grad_()
        oh, ow = (h // 2, w // 2) if pool else (h, w)
        dy = torch.randn(n, c, oh, ow, device="cuda").to(torch.bfloat16)\
            .contiguous(memory_format=torch.channels_last)

        def stock(t):
            y = torch.relu(t + b16.view(1, -1, 1, 1))
            return ops.max_pool_nhwc(y, 2, 2, 0) if pool else y

        def fused(t):
            if pool:
                return ops.bias_relu_pool(t, b32, 2, 2, 0)
            return ops.bias_relu(t, b32)

        def drop_grads():
            xg.grad = None
            b32.grad = None
            b16.grad = None

        def stock_fwd():
            with torch.no_grad():
                stock(x)

        def fused_fwd():
            with torch.no_grad():
                fused(x)

        def stock_fb():
            stock(xg).backward(dy)
            drop_grads()

        def fused_fb():
            fused(xg).backward(dy)
            drop_grads()

        probe = fused(xg)  # a silent fall-back would time the wrong thing
        want = "BiasReLUMaxPoolNHWCFn" if pool else "BiasReLUFn"
        assert want in probe.grad_fn.name()
        del probe
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
        need_fwd = 2 * n_in + 2 * n_out
        need_fb = need_fwd + 4 * n_out + 2 * n_in
        if pool:
            need_fb += 2 * n_out
        r = {"name": name, "shape": [n, c, h, w], "pool": pool,
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
        r["fwd_speedup"] = round(r["stock_fwd_ms"] / r["fused_fwd_ms"], 2)
        r["fb_speedup"] = round(r["stock_fb_ms"] / r["fused_fb_ms"], 2)
        line = json.dumps(r)
        print(line, flush=True)
        lines.append(line)
        del x, xg, dy, b32, b16
        torch.cuda.empty_cache()

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)),
                    exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
