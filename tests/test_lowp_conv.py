"""LowpConv2d on the CPU: it is a stock nn.Conv2d in everything a
checkpoint or an initialisation can see, and with nothing staged its
forward is the stock forward."""
import os
import sys

import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch.nn as nn  # noqa: E402

from kubeshare_amd.models import resnet18, resnet50  # noqa: E402
from kubeshare_amd.models import resnet as R  # noqa: E402
from kubeshare_amd.models.conv import LowpConv2d  # noqa: E402


def test_same_init_and_state_dict_as_stock_conv(monkeypatch):
    torch.manual_seed(0)
    ours = resnet18(num_classes=10)
    monkeypatch.setattr(R, "LowpConv2d", nn.Conv2d)
    torch.manual_seed(0)
    stock = resnet18(num_classes=10)
    assert not any(isinstance(m, LowpConv2d) for m in stock.modules())
    sd_ours, sd_stock = ours.state_dict(), stock.state_dict()
    assert list(sd_ours.keys()) == list(sd_stock.keys())
    for k in sd_ours:
        assert torch.equal(sd_ours[k], sd_stock[k]), k
    stock.load_state_dict(sd_ours)
    ours.load_state_dict(sd_stock)


def test_every_resnet_conv_is_listed_once():
    model = resnet50(num_classes=10)
    convs = [m for m in model.modules() if isinstance(m, nn.Conv2d)]
    assert len(convs) == 53
    assert all(isinstance(m, LowpConv2d) for m in convs)
    assert [id(m) for m in model._lowp_convs] == [id(m) for m in convs]
    assert not any("_lowp" in k for k in model.state_dict())


def test_forward_uses_staged_weight_only_when_present():
    torch.manual_seed(0)
    conv = LowpConv2d(3, 4, 3, padding=1, bias=False)
    x = torch.randn(2, 3, 5, 5)
    ref = nn.functional.conv2d(x, conv.weight, None, 1, 1)
    assert conv._lowp_weight is None
    assert torch.equal(conv(x), ref)
    conv._lowp_weight = conv.weight.detach() * 2
    assert torch.equal(conv(x), nn.functional.conv2d(
        x, conv.weight.detach() * 2, None, 1, 1))
    conv._lowp_weight = None
    assert torch.equal(conv(x), ref)


def test_cpu_autocast_stages_nothing():
    from kubeshare_amd import ops
    model = resnet18(num_classes=10)
    assert ops.stage_lowp_weights(model._lowp_convs) == []
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert ops.stage_lowp_weights(model._lowp_convs) == []
    assert all(m._lowp_weight is None for m in model._lowp_convs)
