"""Max-pool module for the fused path: a stock nn.MaxPool2d (no
parameters, no buffers — state_dict keys of every model stay as they
are) that routes through the NHWC bf16 gfx950 kernels of
kubeshare_amd.ops once ops.fuse_model has flagged it."""
import torch.nn as nn


class FusedMaxPool2d(nn.MaxPool2d):
    fused_ops = False  # set by kubeshare_amd.ops.fuse_model

    def forward(self, x):
        if self.fused_ops and self.dilation == 1 and not self.ceil_mode \
                and not self.return_indices:
            from .. import ops
            # KUBESHARE_FUSED_POOL=0: stock path even when flagged
            if ops.fused_pool_enabled():
                return ops.max_pool_nhwc(x, self.kernel_size, self.stride,
                                         self.padding)
        return super().forward(x)
