"""Per-shape microbench: the stock weight gradient of a stride-1 1x1
convolution (aten::convolution_backward, weight half only: MIOpen's
split-K solver with the zero fill and the cast its invoker wraps around
it) vs ops.wrw_gemm_1x1 (ops/hip/wrw_gemm.hip: the split-K MFMA GEMM and
its reduce kernel), on the 12 distinct stride-1 1x1 shapes of ResNet50 at
batch 256, bf16 channels-last, with the tuned MIOpen db shipped in the
tree. Prints one JSON line per shape and a total (--out also writes them
to a file; the committed record is profiles/wrw_gemm_bench.json).

Timing is tools/dgrad_fwd_bench.py's: `*_ms` is GPU time between device
events around `iters` back-to-back calls with a calibrated ops.burn()
queued first, so both sides are timed with everything they launch; the
two paths run alternately in the same session and the round is repeated.
`winner` is `gemm` or `stock` when that side's slowest round beats the
other's fastest, else `tie`. `plan` is {TM, TN, S, L} of the GEMM;
`min_ms` is the time 8 TB/s needs to read both operands once.
`*_err_over_bound` is each result's largest error against a float64
reference over the elementwise bound of tests/test_wrw_gemm_gpu.py (one
bf16 rounding plus the worst case of an f32 accumulation), at the timed
size."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = [  # (C in, K out, h, weight gradients per ResNet50 step)
    (64, 64, 56, 1), (64, 256, 56, 4), (256, 64, 56, 2), (256, 128, 56, 1),
    (128, 512, 28, 4), (512, 128, 28, 3), (512, 256, 28, 1),
    (256, 1024, 14, 6), (1024, 256, 14, 5), (1024, 512, 14, 1),
    (512, 2048, 7, 3), (2048, 512, 7, 2),
]
HBM_BYTES_PER_MS = 8e9


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
    plan = ops._load().wrw_gemm_plan

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

    lines = []
    total = {"stock": 0.0, "gemm": 0.0}
    torch.manual_seed(0)
    with torch.no_grad():
        for c, k, h, per_step in SHAPES:
            w = rand((k, c, 1, 1))
            x = rand((args.batch, c, h, h))
            dy = rand((args.batch, k, h, h))
            pixels = args.batch * h * h

            def stock():
                return aten.convolution_backward(
                    dy, x, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0],
                    1, [False, True, False])[1]

            def gemm():
                return ops.wrw_gemm_1x1(x, dy)

            # both results against float64, over the bound of
            # tests/test_wrw_gemm_gpu.py
            xr = x.permute(0, 2, 3, 1).reshape(pixels, c).double()
            dyr = dy.permute(0, 2, 3, 1).reshape(pixels, k).double()
            ref = dyr.t() @ xr
            bound = 2.0 ** -8 * ref.abs() + pixels * 2.0 ** -24 * (
                dyr.abs().t() @ xr.abs())

            def over_bound(dw):
                err = (dw.double().reshape(k, c) - ref).abs()
                return round((err / bound).max().item(), 4)

            r = {"name": f"{c}->{k} 1x1 @{h}", "batch": args.batch,
                 "pixels": pixels, "per_step": per_step,
                 "plan": plan(pixels, c, k),
                 "min_ms": round(2 * pixels * (c + k) / HBM_BYTES_PER_MS, 4),
                 "stock_err_over_bound": over_bound(stock()),
                 "gemm_err_over_bound": over_bound(gemm())}
            del xr, dyr, ref, bound
            gpu = measure({"stock": stock, "gemm": gemm})
            for key, ts in gpu.items():
                r[key + "_ms"] = round(statistics.median(ts), 4)
                r[key + "_min_ms"] = round(min(ts), 4)
                r[key + "_max_ms"] = round(max(ts), 4)
                total[key] += per_step * r[key + "_ms"]
            r["speedup"] = round(r["stock_ms"] / r["gemm_ms"], 3)
            r["winner"] = (
                "gemm" if r["gemm_max_ms"] < r["stock_min_ms"] else
                "stock" if r["stock_max_ms"] < r["gemm_min_ms"] else "tie")
            line = json.dumps(r)
            print(line, flush=True)
            lines.append(line)
            del w, x, dy
            torch.cuda.empty_cache()
    line = json.dumps({
        "name": "ResNet50 step, 33 stride-1 1x1 weight gradients",
        "stock_ms_per_step": round(total["stock"], 4),
        "gemm_ms_per_step": round(total["gemm"], 4)})
    print(line, flush=True)
    lines.append(line)

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)),
                    exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
