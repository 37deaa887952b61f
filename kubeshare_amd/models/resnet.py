"""ResNet family for the sharing benchmarks (BASELINE.json: ResNet50 on
synthetic data / random init; the reference's e2e workloads are
torchelastic resnet18/50 + vgg16 pods, test/distribute/**).

Written for MI355X training throughput: channels-last memory format and
bf16 autocast are applied by the caller (bench/worker); the module keeps
to stock conv/bn so MIOpen picks its gfx950 kernels, with the fused
BN+ReLU HIP op from kubeshare_amd.ops swapped in where profitable.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .conv import LowpConv2d
from .pool import FusedMaxPool2d


class Bottleneck(nn.Module):
    expansion = 4
    fused_ops = False  # set by kubeshare_amd.ops.fuse_model

    def __init__(self, in_ch: int, width: int, stride: int = 1):
        super().__init__()
        out_ch = width * self.expansion
        self.conv1 = LowpConv2d(in_ch, width, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = LowpConv2d(width, width, 3, stride=stride, padding=1,
                                bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = LowpConv2d(width, out_ch, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(out_ch)
        self.relu = nn.ReLU(inplace=True)
        self.down = None
        if stride != 1 or in_ch != out_ch:
            self.down = nn.Sequential(
                LowpConv2d(in_ch, out_ch, 1, stride=stride, bias=False),
                nn.BatchNorm2d(out_ch),
            )

    def forward(self, x):
        # a pair (x, x_id) is one activation under two autograd handles
        # (ops.bn_relu(fork=True)): conv1 consumes x, the identity /
        # downsample branch x_id, and a pair comes back. A plain tensor
        # in gives a plain tensor out.
        pair = isinstance(x, tuple)
        x, x_id = x if pair else (x, x)
        if self.fused_ops:
            from .. import ops
            # the downsample BN has no activation and only the join
            # reads it: ops.bn_join runs both BNs, the add and the ReLU
            # as one op (or as two bn_relu calls where it cannot)
            if self.down is not None:
                x_d = self.down[0](x_id)
            out = ops.bn_relu(self.conv1(x), self.bn1)
            out = ops.bn_relu(self.conv2(out), self.bn2)
            if self.down is not None:
                return ops.bn_join(self.conv3(out), self.bn3, x_d,
                                   self.down[1], fork=pair)
            return ops.bn_relu(self.conv3(out), self.bn3, res=x_id,
                               fork=pair)
        identity = x_id if self.down is None else self.down(x_id)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        out = self.relu(out + identity)
        return (out, out) if pair else out


class BasicBlock(nn.Module):
    expansion = 1
    fused_ops = False  # set by kubeshare_amd.ops.fuse_model

    def __init__(self, in_ch: int, width: int, stride: int = 1):
        super().__init__()
        self.conv1 = LowpConv2d(in_ch, width, 3, stride=stride, padding=1,
                                bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = LowpConv2d(width, width, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.relu = nn.ReLU(inplace=True)
        self.down = None
        if stride != 1 or in_ch != width:
            self.down = nn.Sequential(
                LowpConv2d(in_ch, width, 1, stride=stride, bias=False),
                nn.BatchNorm2d(width),
            )

    def forward(self, x):
        pair = isinstance(x, tuple)  # see Bottleneck.forward
        x, x_id = x if pair else (x, x)
        if self.fused_ops:
            from .. import ops
            if self.down is not None:  # see Bottleneck.forward
                x_d = self.down[0](x_id)
            out = ops.bn_relu(self.conv1(x), self.bn1)
            if self.down is not None:
                return ops.bn_join(self.conv2(out), self.bn2, x_d,
                                   self.down[1], fork=pair)
            return ops.bn_relu(self.conv2(out), self.bn2, res=x_id,
                               fork=pair)
        identity = x_id if self.down is None else self.down(x_id)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        out = self.relu(out + identity)
        return (out, out) if pair else out


class ResNet(nn.Module):
    fused_ops = False  # stem BN+ReLU fusion (set by ops.fuse_model)

    def __init__(self, block, layers, num_classes: int = 1000):
        super().__init__()
        self.in_ch = 64
        self.conv1 = LowpConv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = FusedMaxPool2d(3, stride=2, padding=1)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2)
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(512 * block.expansion, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out",
                                        nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
        # every conv of the model, for ops.stage_lowp_weights (a plain
        # list: not a registered submodule container)
        self._lowp_convs = [m for m in self.modules()
                            if isinstance(m, LowpConv2d)]

    def _make_layer(self, block, width, n, stride=1):
        layers = [block(self.in_ch, width, stride)]
        self.in_ch = width * block.expansion
        layers += [block(self.in_ch, width) for _ in range(n - 1)]
        return nn.Sequential(*layers)

    def forward(self, x):
        if not self.fused_ops:
            return self._forward(x)
        from .. import ops
        # one launch casts every conv weight for this forward (bf16
        # autocast only; otherwise nothing is staged and the convs use
        # self.weight); the staged copies are dropped on the way out
        staged = ops.stage_lowp_weights(self._lowp_convs)
        try:
            return self._forward(x)
        finally:
            ops.clear_lowp_weights(staged)

    def _forward(self, x):
        if self.fused_ops:
            from .. import ops
            # the pool module runs the stem's BN+ReLU itself, fused with
            # the pool where it can (ops.bn_relu_pool)
            x = self.maxpool(ops.PendingBNReLU(self.conv1(x), self.bn1))
            if ops.bn_fork_enabled():
                # every block hands its output on as a pair, so the two
                # gradients of a residual join reach the block's last BN
                # separately and are summed inside its backward kernel
                x = (x, x)
        else:
            x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        if isinstance(x, tuple):
            x = x[0]
        x = torch.flatten(self.avgpool(x), 1)
        return self.fc(x)


def resnet18(num_classes: int = 1000) -> ResNet:
    return ResNet(BasicBlock, [2, 2, 2, 2], num_classes)


def resnet50(num_classes: int = 1000) -> ResNet:
    return ResNet(Bottleneck, [3, 4, 6, 3], num_classes)
