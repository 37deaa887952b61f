"""VGG16 — the third workload family of the reference's distributed e2e
suite (test/distribute/**/vgg16*). Conv->BN->ReLU triples are structured
as blocks so kubeshare_amd.ops.fuse_model can route them through the
fused NHWC bf16 BN+ReLU gfx950 kernel (same op the ResNet blocks use).

`vgg16` is the BN variant (torchvision's vgg16_bn layout). The reference
starts the PyTorch ImageNet example with --arch=vgg16, which is the plain
BN-free net: that one is `vgg16_plain` (VGGPlain), with torchvision's
vgg16 layout and state_dict keys."""
import torch.nn as nn

from .conv import LowpConv2d
from .pool import FusedMaxPool2d

_CFG16 = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M",
          512, 512, 512, "M", 512, 512, 512, "M"]


class ConvBNReLU(nn.Module):
    fused_ops = False  # set by kubeshare_amd.ops.fuse_model
    # set by VGG on the blocks directly in front of a pool: when fused,
    # such a block leaves its BN+ReLU to the pool module
    # (ops.PendingBNReLU -> ops.bn_relu_pool)
    defer_to_pool = False

    def __init__(self, in_ch: int, out_ch: int):
        super().__init__()
        self.conv = nn.Conv2d(in_ch, out_ch, 3, padding=1)
        self.bn = nn.BatchNorm2d(out_ch)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        if self.fused_ops:
            from .. import ops
            if self.defer_to_pool:
                return ops.PendingBNReLU(self.conv(x), self.bn)
            return ops.bn_relu(self.conv(x), self.bn)
        return self.relu(self.bn(self.conv(x)))


class VGG(nn.Module):
    def __init__(self, cfg, num_classes: int = 1000):
        super().__init__()
        layers, in_ch = [], 3
        for v in cfg:
            if v == "M":
                layers[-1].defer_to_pool = True
                layers.append(FusedMaxPool2d(2, 2))
            else:
                layers.append(ConvBNReLU(in_ch, v))
                in_ch = v
        self.features = nn.Sequential(*layers)
        self.avgpool = nn.AdaptiveAvgPool2d(7)
        self.classifier = nn.Sequential(
            nn.Linear(512 * 7 * 7, 4096), nn.ReLU(True), nn.Dropout(),
            nn.Linear(4096, 4096), nn.ReLU(True), nn.Dropout(),
            nn.Linear(4096, num_classes))

    def forward(self, x):
        x = self.avgpool(self.features(x)).flatten(1)
        return self.classifier(x)


def vgg16(num_classes: int = 1000) -> VGG:
    return VGG(_CFG16, num_classes)


class VGGPlain(nn.Module):
    """torchvision's plain VGG (no BatchNorm): conv(+bias) -> ReLU pairs,
    a 2x2 max-pool after some of them. `features` is a flat nn.Sequential
    with torchvision's indices, so its checkpoints load.

    Stock forward: the modules as they stand. Once ops.fuse_model has
    flagged the model (and unless KUBESHARE_BIAS_RELU=0), the forward of
    a GPU input walks `features` itself: each conv runs WITHOUT its bias, and the
    bias, the ReLU and, where one follows, the pool run as one op
    (ops.bias_relu / ops.bias_relu_pool)."""
    fused_ops = False  # set by kubeshare_amd.ops.fuse_model

    def __init__(self, cfg, num_classes: int = 1000):
        super().__init__()
        layers, in_ch = [], 3
        for v in cfg:
            if v == "M":
                layers.append(FusedMaxPool2d(2, 2))
            else:
                layers += [LowpConv2d(in_ch, v, 3, padding=1),
                           nn.ReLU(inplace=True)]
                in_ch = v
        self.features = nn.Sequential(*layers)
        self.avgpool = nn.AdaptiveAvgPool2d(7)
        self.classifier = nn.Sequential(
            nn.Linear(512 * 7 * 7, 4096), nn.ReLU(True), nn.Dropout(),
            nn.Linear(4096, 4096), nn.ReLU(True), nn.Dropout(),
            nn.Linear(4096, num_classes))
        # every conv of the model, for ops.stage_lowp_weights (a plain
        # list: not a registered submodule container)
        self._lowp_convs = [m for m in self.modules()
                            if isinstance(m, LowpConv2d)]

    def forward(self, x):
        # GPU inputs only: on the CPU every fused op would fall back to
        # eager anyway, and a bias-free conv followed by a separate add
        # rounds differently from the conv's own bias epilogue there, so
        # the stock modules are the better fall-back
        if self.fused_ops and x.is_cuda:
            from .. import ops
            if ops.bias_relu_enabled():
                # one launch casts every conv weight for this forward
                # (see ResNet.forward); dropped on the way out
                staged = ops.stage_lowp_weights(self._lowp_convs)
                try:
                    x = self._fused_features(x, ops)
                finally:
                    ops.clear_lowp_weights(staged)
                return self.classifier(self.avgpool(x).flatten(1))
        return self.classifier(self.avgpool(self.features(x)).flatten(1))

    @staticmethod
    def _pool_fusable(m, ops):
        """The conditions FusedMaxPool2d.forward tests before it takes
        the fused path."""
        return (isinstance(m, FusedMaxPool2d) and m.fused_ops
                and m.dilation == 1 and not m.ceil_mode
                and not m.return_indices and ops.fused_pool_enabled())

    def _fused_features(self, x, ops):
        mods = list(self.features)
        i, n = 0, len(mods)
        while i < n:
            m = mods[i]
            if isinstance(m, LowpConv2d) and m.bias is not None \
                    and i + 1 < n and isinstance(mods[i + 1], nn.ReLU):
                w = m._lowp_weight if m._lowp_weight is not None \
                    else m.weight
                x = m._conv_forward(x, w, None)
                nxt = mods[i + 2] if i + 2 < n else None
                if self._pool_fusable(nxt, ops):
                    x = ops.bias_relu_pool(x, m.bias, nxt.kernel_size,
                                           nxt.stride, nxt.padding)
                    i += 3
                else:
                    x = ops.bias_relu(x, m.bias)
                    i += 2
            else:
                x = m(x)
                i += 1
        return x


def vgg16_plain(num_classes: int = 1000) -> VGGPlain:
    return VGGPlain(_CFG16, num_classes)
