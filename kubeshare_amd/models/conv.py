"""Conv module for the fused path: a stock nn.Conv2d (same constructor,
same parameters and state_dict keys, same init RNG order) whose forward
uses a staged low-precision copy of its weight when one is present.

Under bf16 autocast every conv casts its f32 master weight to bf16 with
a launch of its own, and autograd casts each weight gradient back with
another. The model's forward instead stages ALL conv weights with one
multi-tensor cast (ops.stage_lowp_weights) before the first conv and
clears the staged references when it returns; the matching backward
node casts all weight gradients back in one launch.

With a staged weight the convolution itself goes through
ops.conv2d_split where that op applies: the same ATen convolution, whose
backward issues the weight gradient on a side stream. The staged
weight's CastWeightsFn node is downstream of every such gradient and
joins the side stream before it reads them. Where ops.fuse_model has
flagged the conv (_dgrad_fwd) the staged weight comes with its mirror,
and conv2d_split runs the data gradient as a forward convolution."""
import torch
import torch.nn as nn


class LowpConv2d(nn.Conv2d):
    # a bf16 copy of self.weight for the forward in progress, or None
    # (plain attribute: never a parameter, a buffer or a state_dict key)
    _lowp_weight = None
    # set by ops.fuse_model: the data gradient of this conv runs as a
    # forward convolution of dy with _lowp_mirror, the mirrored staged
    # weight that ops.stage_lowp_weights then provides beside _lowp_weight
    _dgrad_fwd = False
    _lowp_mirror = None

    def _split_input(self, x, w):
        """x as ops.conv2d_split takes it, or None for the stock path:
        CUDA bf16 x and weight, no bias, zero padding given as numbers,
        and KUBESHARE_WRW_STREAM not 0. An x of another floating dtype
        is cast as autocast would cast it for F.conv2d."""
        if self.bias is not None or self.padding_mode != "zeros" \
                or isinstance(self.padding, str):
            return None
        if not (w.is_cuda and x.is_cuda and w.dtype == torch.bfloat16
                and x.dim() == 4):
            return None
        from .. import ops
        if not ops.wrw_stream_enabled():
            return None
        if x.dtype != torch.bfloat16:
            if not (x.is_floating_point()
                    and torch.is_autocast_enabled("cuda")
                    and torch.get_autocast_dtype("cuda") == torch.bfloat16):
                return None
            x = x.to(torch.bfloat16)
        return x

    def forward(self, x):
        w = self._lowp_weight
        if w is None:
            return super().forward(x)
        xs = self._split_input(x, w)
        if xs is None:
            return self._conv_forward(x, w, self.bias)
        from .. import ops
        return ops.conv2d_split(xs, w, self.stride, self.padding,
                                self.dilation, self.groups,
                                self._lowp_mirror)
