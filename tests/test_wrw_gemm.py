"""The 1x1 weight-gradient GEMM on the CPU: the KUBESHARE_WRW_GEMM switch,
the eligibility predicate, and LowpConv2d without a staged weight."""
import os
import sys

import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from kubeshare_amd import ops  # noqa: E402
from kubeshare_amd.models.conv import LowpConv2d  # noqa: E402


@pytest.mark.parametrize("value,want", [(None, False), ("1", True),
                                        ("0", False), ("", False)])
def test_switch_follows_the_environment(monkeypatch, value, want):
    if value is None:
        monkeypatch.delenv("KUBESHARE_WRW_GEMM", raising=False)
    else:
        monkeypatch.setenv("KUBESHARE_WRW_GEMM", value)
    assert ops.wrw_gemm_enabled() is want


@pytest.mark.parametrize("dtype,cin,k,stride,padding,groups", [
    (torch.bfloat16, 16, 1, 1, 0, 1),   # eligible but for the device
    (torch.float32, 16, 1, 1, 0, 1),
    (torch.bfloat16, 16, 3, 1, 1, 1),
    (torch.bfloat16, 16, 1, 2, 0, 1),
    (torch.bfloat16, 16, 1, 1, 1, 1),
    (torch.bfloat16, 16, 1, 1, 0, 2),
    (torch.bfloat16, 12, 1, 1, 0, 1),
])
def test_predicate_is_false_off_the_gpu(dtype, cin, k, stride, padding,
                                        groups):
    x = torch.zeros(2, cin, 4, 4, dtype=dtype)
    w = torch.zeros(16, cin // groups, k, k, dtype=dtype)
    assert not ops.wrw_gemm_supported(x, w, stride, padding, 1, groups)
    assert not ops.wrw_gemm_supported(x, w, (stride, stride),
                                      (padding, padding), (1, 1), groups)


def test_lowp_conv_without_a_staged_weight_is_the_stock_conv(monkeypatch):
    monkeypatch.setenv("KUBESHARE_WRW_GEMM", "1")
    monkeypatch.setattr(ops, "_ext", None)
    torch.manual_seed(0)
    conv = LowpConv2d(8, 16, 1, bias=False)
    x = torch.randn(2, 8, 4, 4)
    y = conv(x)
    assert y.grad_fn.name() == "ConvolutionBackward0"
    assert torch.equal(y, torch.nn.functional.conv2d(x, conv.weight))
    assert ops._ext is None  # the extension was not asked for
