"""Per-shape microbench: the stock data gradient of a stride-1
convolution (aten::convolution_backward, data half only) vs the forward
convolution of dy with the mirrored weight that
ops.conv2d_split(mirror=...) runs instead, on the 13 ResNet50 shapes the
default routing covers, at batch 256, bf16 channels-last, with the tuned
MIOpen db shipped in the tree. A last line times the mirror launch
itself (ops.mirror_weights) for ResNet50's full list of routed weights.
Event-timed after warm-up; the two paths run alternately in the same
session and the round is repeated so the spread is visible. Prints one
JSON line per shape (--out also writes them to a file; the committed
record is profiles/dgrad_fwd_bench.json).

Timing is tools/bn_join_bench.py's: `*_ms` is GPU time between device
events around `iters` back-to-back calls with a calibrated ops.burn()
queued first. `wins` is true when the mirrored forward's slowest round
is faster than the stock data gradient's fastest round.

The shapes are named as the data gradient sees them: `reads` channels of
dy in, `writes` channels of dx out, kernel k, at h x h."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = [  # (reads, writes, k, h, data gradients per ResNet50 step)
    (64, 256, 1, 56, 2), (256, 64, 1, 56, 4), (64, 64, 1, 56, 1),
    (128, 512, 1, 28, 3), (512, 128, 1, 28, 4),
    (256, 1024, 1, 14, 5), (1024, 256, 1, 14, 6),
    (512, 2048, 1, 7, 2), (2048, 512, 1, 7, 3),
    (64, 64, 3, 56, 3), (128, 128, 3, 28, 3), (256, 256, 3, 14, 5),
    (512, 512, 3, 7, 2),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the lines here")
    args = ap.parse_args()

    from kubeshare_amd.utils.tuning import apply_miopen_tuning
    apply_miopen_tuning()
    import torch
    from kubeshare_amd import ops

    sync = torch.cuda.synchronize
    aten = torch.ops.aten

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

    def measure(fns):
        """{key: [primed GPU ms per round]} with the paths alternated."""
        iters, host_ms = {}, {}
        for key, fn in fns.items():
            for _ in range(args.warmup):
                fn()
            sync()
            t, hms = timed(fn, 20)
            iters[key] = max(20, min(2000, int(args.window_ms / t) + 1))
            host_ms[key] = hms
        gpu = {key: [] for key in fns}
        for _ in range(args.repeats):
            for key, fn in fns.items():
                prime = 1.5 * host_ms[key] * iters[key] + 1.0
                t, hms = timed(fn, iters[key], prime)
                host_ms[key] = max(host_ms[key], hms)
                gpu[key].append(t)
        return gpu

    def stats(r, key, ts):
        r[key + "_ms"] = round(statistics.median(ts), 4)
        r[key + "_min_ms"] = round(min(ts), 4)
        r[key + "_max_ms"] = round(max(ts), 4)

    lines = []
    saved = 0.0
    with torch.no_grad():
        for reads, writes, k, h, per_step in SHAPES:
            p = k // 2
            # the forward conv is writes -> reads channels: W (reads,
            # writes, k, k), x (N, writes, h, h), dy (N, reads, h, h)
            w = rand((reads, writes, k, k))
            x = rand((args.batch, writes, h, h))
            dy = rand((args.batch, reads, h, h))
            (wm,) = ops.mirror_weights([w])

            def stock():
                return aten.convolution_backward(
                    dy, x, w, None, [1, 1], [p, p], [1, 1], False, [0, 0],
                    1, [True, False, False])[0]

            def mirrored():
                return aten.convolution(dy, wm, None, [1, 1],
                                        [k - 1 - p, k - 1 - p], [1, 1],
                                        False, [0, 0], 1)

            gpu = measure({"dgrad": stock, "mirrored_fwd": mirrored})
            r = {"name": f"{reads}->{writes} {k}x{k} @{h}",
                 "batch": args.batch, "per_step": per_step}
            for key, ts in gpu.items():
                stats(r, key, ts)
            r["speedup"] = round(r["dgrad_ms"] / r["mirrored_fwd_ms"], 3)
            r["wins"] = r["mirrored_fwd_max_ms"] < r["dgrad_min_ms"]
            r["saved_ms_per_step"] = round(
                per_step * (r["dgrad_ms"] - r["mirrored_fwd_ms"]), 4)
            saved += r["saved_ms_per_step"]
            line = json.dumps(r)
            print(line, flush=True)
            lines.append(line)
            del w, x, dy, wm
            torch.cuda.empty_cache()

        # the mirror launch for the whole network
        from kubeshare_amd.models import resnet50
        model = ops.fuse_model(resnet50()).cuda().to(
            memory_format=torch.channels_last)
        ws = [m.weight.detach().to(torch.bfloat16)
              for m in model._lowp_convs if m._dgrad_fwd]
        gpu = measure({"mirror": lambda: ops.mirror_weights(ws)})
        elems = sum(t.numel() for t in ws)
        r = {"name": "mirror_weights, ResNet50 routed list",
             "tensors": len(ws), "elements": elems,
             "moved_mb": round(4 * elems / 1e6, 1)}
        stats(r, "mirror", gpu["mirror"])
        r["gbs"] = round(4 * elems / r["mirror_ms"] / 1e6, 1)
        r["net_saved_ms_per_step"] = round(saved - r["mirror_ms"], 4)
        line = json.dumps(r)
        print(line, flush=True)
        lines.append(line)

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)),
                    exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
