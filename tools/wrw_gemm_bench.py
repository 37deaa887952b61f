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
size.

--shapes conv (or all) adds the ten other distinct conv shapes of ResNet50
but the stem, 3x3 at stride 1 and 2 and 1x1 at stride 2, for which the
GEMM side is ops.wrw_gemm_conv (the same engine with a gathered x operand)
and the bound is that of tests/test_wrw_gemm_conv_gpu.py; the committed
record of those rows is profiles/wrw_gemm_conv_bench.json."""
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
CONV_SHAPES = [  # (C in, K out, input h, per step, kernel, stride)
    (64, 64, 56, 3, 3, 1), (128, 128, 28, 3, 3, 1), (256, 256, 14, 5, 3, 1),
    (512, 512, 7, 2, 3, 1),
    (128, 128, 56, 1, 3, 2), (256, 256, 28, 1, 3, 2), (512, 512, 14, 1, 3, 2),
    (256, 512, 56, 1, 1, 2), (512, 1024, 28, 1, 1, 2),
    (1024, 2048, 14, 1, 1, 2),
]
HBM_BYTES_PER_MS = 8e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", choices=("1x1", "conv", "all"),
                    default="1x1", help="stride-1 1x1 (default), the 3x3 "
                    "and stride-2 shapes, or both")
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

    def weight_grad_f64(x64, dy64, ker, st, pad):
        """dW (K, C, ker, ker) in float64: one GEMM per tap over the
        strided window of the zero-padded x that the tap reads."""
        ho, wo = dy64.shape[2:]
        xp = torch.nn.functional.pad(x64, (pad, pad, pad, pad))
        dyr = dy64.permute(1, 0, 2, 3).reshape(dy64.shape[1], -1)
        taps = [dyr @ xp[:, :, r:r + st * ho:st, s:s + st * wo:st]
                .permute(0, 2, 3, 1).reshape(-1, x64.shape[1])
                for r in range(ker) for s in range(ker)]
        return torch.stack(taps, -1).view(dy64.shape[1], x64.shape[1], ker,
                                          ker)

    shapes = []
    if args.shapes in ("1x1", "all"):
        shapes += [s + (1, 1) for s in SHAPES]
    if args.shapes in ("conv", "all"):
        shapes += CONV_SHAPES
    lines = []
    total = {"stock": 0.0, "gemm": 0.0}
    torch.manual_seed(0)
    with torch.no_grad():
        for c, k, h, per_step, ker, st in shapes:
            pad = ker // 2
            ho = (h + 2 * pad - ker) // st + 1
            w = rand((k, c, ker, ker))
            x = rand((args.batch, c, h, h))
            dy = rand((args.batch, k, ho, ho))
            pixels = args.batch * ho * ho  # the reduction length

            def stock():
                return aten.convolution_backward(
                    dy, x, w, None, [st, st], [pad, pad], [1, 1], False,
                    [0, 0], 1, [False, True, False])[1]

            def gemm():
                return ops.wrw_gemm_conv(x, dy, ker, st, pad)

            # both results against float64, over the bound of
            # tests/test_wrw_gemm_gpu.py and tests/test_wrw_gemm_conv_gpu.py
            ref = weight_grad_f64(x.double(), dy.double(), ker, st, pad)
            bound = 2.0 ** -8 * ref.abs() + pixels * 2.0 ** -24 * \
                weight_grad_f64(x.double().abs(), dy.double().abs(), ker, st,
                                pad)

            def over_bound(dw):
                err = (dw.double() - ref).abs()
                return round((err / bound).max().item(), 4)

            name = f"{c}->{k} {ker}x{ker} @{h}" + (f"->{ho}" if st > 1 else "")
            r = {"name": name, "batch": args.batch,
                 "pixels": pixels, "per_step": per_step,
                 "plan": plan(pixels, c, k, ker * ker),
                 "min_ms": round(2 * (args.batch * h * h * c + pixels * k)
                                 / HBM_BYTES_PER_MS, 4),
                 "stock_err_over_bound": over_bound(stock()),
                 "gemm_err_over_bound": over_bound(gemm())}
            del ref, bound
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
        "name": "ResNet50 step, %d weight gradients (--shapes %s)" % (
            sum(s[3] for s in shapes), args.shapes),
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
