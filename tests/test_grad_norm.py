"""Argument handling around the gradient-norm kernels, without a GPU."""
import os
import sys

import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from kubeshare_amd import ops  # noqa: E402


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_grad_norm_on_cpu_tensors(dtype):
    g = torch.Generator().manual_seed(3)
    ts = [torch.randn(5, 7, generator=g).to(dtype), None,
          torch.randn(4, 3, 2, 2, generator=g).to(dtype).contiguous(
              memory_format=torch.channels_last),
          torch.zeros(3, dtype=dtype)]
    total, each = ops.grad_norm(ts, per_tensor=True)
    want = torch.stack([torch.zeros(()) if t is None
                        else torch.linalg.vector_norm(t.float()) for t in ts])
    assert total.dtype == each.dtype == torch.float32 and total.dim() == 0
    torch.testing.assert_close(each, want)
    torch.testing.assert_close(total, torch.linalg.vector_norm(want))
    assert ops.grad_norm([None]).item() == 0.0
    with pytest.raises(ValueError):  # mixed dtypes
        ops.grad_norm([ts[0], ts[0].to(torch.float64)])
    with pytest.raises(ValueError):  # not dense
        ops.grad_norm([ts[0][:, ::2]])


@pytest.mark.parametrize("kw", [
    {"max_grad_norm": 0.0}, {"max_grad_norm": -1.0},
    {"max_grad_norm": float("inf")}, {"max_grad_norm": float("nan")},
    {"lars": 0.0}, {"lars": -0.5}, {"lars": float("inf")},
    {"lars": 0.5, "lars_eps": float("nan")}])
def test_fused_sgd_rejects_bad_arguments(kw):
    p = torch.zeros(4, requires_grad=True)
    with pytest.raises(ValueError):
        ops.FusedSGD([p], lr=0.1, **kw)


@pytest.mark.parametrize("flags", [["--clip-grad-norm", "1.0"],
                                   ["--lars", "0.001"]])
def test_bench_worker_flags_need_fused_sgd(monkeypatch, capsys, flags):
    from kubeshare_amd import bench_worker
    monkeypatch.setattr(sys, "argv", ["bench_worker"] + flags)
    with pytest.raises(SystemExit) as exc:
        bench_worker.main()
    assert exc.value.code == 2
    assert "--fused-sgd" in capsys.readouterr().err
