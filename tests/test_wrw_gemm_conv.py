"""The 3x3 / stride-2 weight-gradient GEMM on the CPU: the values of the
KUBESHARE_WRW_GEMM switch and the eligibility predicate."""
import os
import sys

import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from kubeshare_amd import ops  # noqa: E402


@pytest.mark.parametrize("value,mode", [(None, "0"), ("0", "0"), ("1", "1"),
                                        ("all", "all")])
def test_mode_follows_the_environment(monkeypatch, value, mode):
    if value is None:
        monkeypatch.delenv("KUBESHARE_WRW_GEMM", raising=False)
    else:
        monkeypatch.setenv("KUBESHARE_WRW_GEMM", value)
    assert ops.wrw_gemm_mode() == mode
    assert ops.wrw_gemm_enabled() is (mode != "0")


@pytest.mark.parametrize("dtype,cin,k,stride,padding,dilation,groups", [
    (torch.bfloat16, 16, 3, 1, 1, 1, 1),   # eligible but for the device
    (torch.bfloat16, 16, 1, 2, 0, 1, 1),   # likewise
    (torch.float32, 16, 3, 1, 1, 1, 1),
    (torch.bfloat16, 16, 5, 1, 2, 1, 1),
    (torch.bfloat16, 16, 3, 1, 2, 2, 1),
    (torch.bfloat16, 16, 3, 1, 1, 1, 2),
    (torch.bfloat16, 12, 3, 1, 1, 1, 1),
])
def test_predicate_is_false_off_the_gpu(dtype, cin, k, stride, padding,
                                        dilation, groups):
    x = torch.zeros(2, cin, 4, 4, dtype=dtype)
    w = torch.zeros(16, cin // groups, k, k, dtype=dtype)
    assert not ops.wrw_gemm_conv_supported(x, w, stride, padding, dilation,
                                           groups)
    assert not ops.wrw_gemm_conv_supported(
        x, w, (stride, stride), (padding, padding), (dilation, dilation),
        groups)
