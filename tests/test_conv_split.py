"""conv2d_split on the CPU: the switch predicate, LowpConv2d's fall-back
to the stock convolution, and tools/trace_overlap.py on a trace small
enough to work out by hand."""
import os
import sys

import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch.nn as nn  # noqa: E402

from kubeshare_amd import ops  # noqa: E402
from kubeshare_amd.models.conv import LowpConv2d  # noqa: E402


def test_switch_predicate(monkeypatch):
    monkeypatch.delenv("KUBESHARE_WRW_STREAM", raising=False)
    assert ops.wrw_stream_enabled()
    for v, want in (("0", False), ("1", True), ("", True), ("off", True)):
        monkeypatch.setenv("KUBESHARE_WRW_STREAM", v)
        assert ops.wrw_stream_enabled() is want


def test_join_without_the_extension_is_a_noop(monkeypatch):
    monkeypatch.setattr(ops, "_ext", None)

    def boom():
        raise AssertionError("wgrad_join must not load the extension")

    monkeypatch.setattr(ops, "_load", boom)
    ops.wgrad_join()


def test_lowp_conv_falls_back_on_cpu_and_without_the_extension(monkeypatch):
    """CPU tensors never reach the extension, staged weight or not: with
    the extension unloadable the forward and backward still run, on the
    stock autograd node."""
    def boom():
        raise ImportError("kubeshare_amd.ops extension not built")

    monkeypatch.setattr(ops, "_ext", None)
    monkeypatch.setattr(ops, "_load", boom)
    monkeypatch.delenv("KUBESHARE_WRW_STREAM", raising=False)
    torch.manual_seed(0)
    conv = LowpConv2d(3, 4, 3, padding=1, bias=False)
    x = torch.randn(2, 3, 5, 5, requires_grad=True)
    for staged in (conv.weight.detach().clone().requires_grad_(),
                   conv.weight.detach().to(torch.bfloat16).requires_grad_()):
        conv._lowp_weight = staged
        xin = x.to(staged.dtype)
        y = conv(xin)
        assert y.grad_fn.name() == "ConvolutionBackward0"
        assert torch.equal(y, nn.functional.conv2d(xin, staged, None, 1, 1))
        y.float().sum().backward()
        assert staged.grad is not None and staged.grad.shape == staged.shape
    conv._lowp_weight = None
    assert conv(x).grad_fn.name() == "ConvolutionBackward0"


def test_split_input_predicate_on_cpu():
    conv = LowpConv2d(3, 4, 3, padding=1, bias=False)
    w = conv.weight.detach().to(torch.bfloat16)
    x = torch.randn(2, 3, 5, 5).to(torch.bfloat16)
    assert conv._split_input(x, w) is None  # CPU
    biased = LowpConv2d(3, 4, 3, padding=1, bias=True)
    assert biased._split_input(x, w) is None
    same = LowpConv2d(3, 4, 3, padding="same", bias=False)
    assert same._split_input(x, w) is None
    refl = LowpConv2d(3, 4, 3, padding=1, padding_mode="reflect", bias=False)
    assert refl._split_input(x, w) is None


# ------------------------------------------------------ trace_overlap.py
# Five dispatches, times in ns. One step = everything up to and including
# the optimizer kernel.
#
#   A  conv_dgrad      [   0, 100)
#   B  zero_ws         [  50,  70)   inside A
#   C  igemm_wrw_x     [  90, 150)   overlaps A on [90, 100), D on [140, 150)
#   D  bn_bwd          [ 140, 200)
#   E  sgd_mom_multi   [ 300, 310)   alone, after a gap
#
#   sum   = 100 + 20 + 60 + 60 + 10 = 250
#   union = [0, 200) + [300, 310)    = 210
#   two or more kernels run on [50, 70) + [90, 100) + [140, 150) = 40
#   zero_ws   : 1 call, total 20, all 20 beside another kernel
#   igemm_wrw : 1 call, total 60, 10 + 10 = 20 beside another kernel
#   conv_dgrad: 1 call, total 100, 20 + 10 = 30 beside another kernel
#   sgd_mom   : 1 call, total 10, 0 beside another kernel
CSV = """\
"Kind","Agent_Id","Queue_Id","Stream_Id","Thread_Id","Dispatch_Id","Kernel_Id","Kernel_Name","Correlation_Id","Start_Timestamp","End_Timestamp"
"KERNEL_DISPATCH","Agent 4",1,1,77,1,10,"conv_dgrad",1,1000,1100
"KERNEL_DISPATCH","Agent 4",2,2,77,3,12,"igemm_wrw_x",3,1090,1150
"KERNEL_DISPATCH","Agent 4",2,2,77,2,11,"zero_ws",2,1050,1070
"KERNEL_DISPATCH","Agent 4",1,1,77,4,13,"bn_bwd",4,1140,1200
"KERNEL_DISPATCH","Agent 4",1,1,77,5,14,"sgd_mom_multi_f32_kernel",5,1300,1310
"""


@pytest.fixture
def trace(tmp_path):
    p = tmp_path / "t_kernel_trace.csv"
    p.write_text(CSV)
    return str(p)


def test_trace_overlap_by_hand(trace):
    import trace_overlap as T

    rows = T.load(trace)
    assert [r[0] for r in rows] == ["conv_dgrad", "zero_ws", "igemm_wrw_x",
                                    "bn_bwd", "sgd_mom_multi_f32_kernel"]
    steps = T.split_steps(rows, "sgd_mom")
    assert len(steps) == 1 and len(steps[0]) == 5
    names = ["zero_ws", "igemm_wrw", "conv_dgrad", "sgd_mom"]
    a = T.analyse(steps[0], names)
    assert a["dispatches"] == 5
    assert a["sum"] == 250
    assert a["union"] == 210
    assert a["names"]["zero_ws"] == {"calls": 1, "total": 20,
                                     "overlapped": 20}
    assert a["names"]["igemm_wrw"] == {"calls": 1, "total": 60,
                                       "overlapped": 20}
    assert a["names"]["conv_dgrad"] == {"calls": 1, "total": 100,
                                        "overlapped": 30}
    assert a["names"]["sgd_mom"] == {"calls": 1, "total": 10,
                                     "overlapped": 0}


def test_trace_overlap_steps_and_cli(trace, tmp_path, capsys):
    import trace_overlap as T

    # two steps (the second shifted by 1000 ns, its optimizer in two
    # launches) and an unfinished third, which is dropped
    rows = T.load(trace)
    second = [(n, s + 1000, e + 1000) for n, s, e in rows]
    second.append(("sgd_mom_multi_f32_kernel", 2312, 2320))
    tail = [("conv_dgrad", 3000, 3100)]
    steps = T.split_steps(rows + second + tail, "sgd_mom")
    assert [len(s) for s in steps] == [5, 6]
    b = T.analyse(steps[1], ["sgd_mom"])
    assert b["sum"] == 258 and b["union"] == 218
    assert b["names"]["sgd_mom"] == {"calls": 2, "total": 18,
                                     "overlapped": 0}
    # touching intervals do not overlap
    c = T.analyse([("a", 0, 10), ("b", 10, 20)], ["a"])
    assert c["union"] == 20 and c["names"]["a"]["overlapped"] == 0

    # names after the options, as the tool's docstring shows them
    assert T.main([trace, "--skip", "0", "zero_ws", "igemm_wrw"]) == 0
    out = capsys.readouterr().out
    assert "union" in out and "igemm_wrw: calls 1.0" in out
    assert "(1 steps)" in out
    assert T.main([trace, "--step-kernel", "no_such_kernel"]) == 1
