"""Conv module for the fused path: a stock nn.Conv2d (same constructor,
same parameters and state_dict keys, same init RNG order) whose forward
uses a staged low-precision copy of its weight when one is present.

Under bf16 autocast every conv casts its f32 master weight to bf16 with
a launch of its own, and autograd casts each weight gradient back with
another. The model's forward instead stages ALL conv weights with one
multi-tensor cast (ops.stage_lowp_weights) before the first conv and
clears the staged references when it returns; the matching backward
node casts all weight gradients back in one launch."""
import torch.nn as nn


class LowpConv2d(nn.Conv2d):
    # a bf16 copy of self.weight for the forward in progress, or None
    # (plain attribute: never a parameter, a buffer or a state_dict key)
    _lowp_weight = None

    def forward(self, x):
        w = self._lowp_weight
        if w is None:
            return super().forward(x)
        return self._conv_forward(x, w, self.bias)
