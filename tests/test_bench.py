"""bench.py contract tests on CPU (plumbing only: tiny model, fp32,
no GPU, gloo for the distributed path)."""
import json
import os
import socket
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TINY = ["--model", "resnet18", "--batch", "2", "--image-size", "64",
        "--steps", "1", "--warmup", "0", "--device", "cpu",
        "--dtype", "fp32", "--use-ops", "off"]


def _parse_json_line(stdout: str) -> dict:
    for line in stdout.splitlines():
        if line.startswith("{"):
            return json.loads(line)
    raise AssertionError(f"no JSON line in output:\n{stdout}")


def test_bench_single(native_bins):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1"] + TINY,
                       cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = _parse_json_line(r.stdout)
    for key in ["metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config"]:
        assert key in out, key
    assert out["n_gpus"] == 1
    assert out["value"] > 0
    assert out["data"] == "synthetic"
    assert out["config"]["pods_per_gpu"] == 2
    assert out["config"]["gpu_request"] == 0.5


def test_bench_dump_outputs(native_bins, tmp_path):
    """--dump-outputs writes each pod's last-step loss, logits and
    non-conv parameters as float32 .npy; --full is accepted and leaves the
    result line as it is. The dumped step starts from the seeded initial
    state, so a run of 1 step and a run of 1+3 steps dump the same
    arrays (fp32 on CPU: equal to accumulated rounding, 1e-4 absolute on
    O(1) values, where a single training step moves them by 1e-1)."""
    import numpy as np
    keys = ("loss", "logits", "params_sample")
    runs = []
    for tag, extra in (("a", []), ("b", ["--steps", "3", "--warmup", "1"])):
        d = tmp_path / f"dump_{tag}"
        r = subprocess.run([sys.executable, "bench.py", "--gpus", "1",
                            "--full", "--dump-outputs", str(d)] + TINY
                           + extra, cwd=REPO, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        out = _parse_json_line(r.stdout)
        assert out["steps"] == (3 if extra else 1)
        assert out["ms_per_step"] > 0
        assert sorted(p.name for p in d.iterdir()) == sorted(
            f"pod0-{i}.{k}.npy" for i in range(2) for k in keys)
        total = 0
        pods = []
        for i in range(2):
            arrs = {k: np.load(d / f"pod0-{i}.{k}.npy") for k in keys}
            assert all(a.dtype == np.float32 for a in arrs.values())
            assert all(np.isfinite(a).all() for a in arrs.values())
            assert arrs["loss"].shape == (1,)
            assert arrs["logits"].shape == (2, 1000)  # batch 2, 1000 classes
            # resnet18's BN + fc parameters: fewer than the sample cap
            assert arrs["params_sample"].shape == (522600,)
            # the dumped loss is the one the result line reports
            assert abs(arrs["loss"][0]
                       - out["config"]["per_pod_loss"][i]) < 1e-3
            total += sum(a.nbytes for a in arrs.values())
            pods.append(arrs)
        assert total <= 64 * 1024 * 1024
        runs.append(pods)
    for pa, pb in zip(*runs):
        for k in keys:
            diff = np.abs(pa[k].astype(np.float64) - pb[k]).max()
            print(k, "max abs diff between runs:", diff)
            assert diff <= 1e-4, (k, diff)


def test_bench_dist2_gloo(native_bins):
    port = socket.socket()
    port.bind(("127.0.0.1", 0))
    p = port.getsockname()[1]
    port.close()
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", str(p), "bench.py", "--gpus", "2"] + TINY,
        cwd=REPO, capture_output=True, text=True, timeout=900,
        env=dict(os.environ, MASTER_ADDR="127.0.0.1"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    out = _parse_json_line(r.stdout)
    assert out["n_gpus"] == 2
    # 2 ranks x 2 pods x 1 step x batch 2 images aggregated
    assert out["config"]["global_batch"] == 8


def test_bench_dist8_gloo(native_bins):
    """8-rank readiness on CPU: the first 8-GPU driver
    run must not be burned on plumbing. 8 ranks x 2 pods = 16 worker
    processes + 8 gpu-schd + 16 pod-mgr over deterministic UDS paths."""
    port = socket.socket()
    port.bind(("127.0.0.1", 0))
    p = port.getsockname()[1]
    port.close()
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
         "--master-port", str(p), "bench.py", "--gpus", "8"] + TINY,
        cwd=REPO, capture_output=True, text=True, timeout=1800,
        env=dict(os.environ, MASTER_ADDR="127.0.0.1"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    out = _parse_json_line(r.stdout)
    assert out["n_gpus"] == 8
    assert out["config"]["global_batch"] == 32  # 8 x 2 pods x batch 2
    assert out["value"] > 0
