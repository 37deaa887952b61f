"""Max-pool module for the fused path: a stock nn.MaxPool2d (no
parameters, no buffers — state_dict keys of every model stay as they
are) that routes through the NHWC bf16 gfx950 kernels of
kubeshare_amd.ops once ops.fuse_model has flagged it.

A fused model may hand it an ops.PendingBNReLU instead of a tensor: the
BN+ReLU directly in front of the pool, not yet run. The flagged module
then runs all three as one op (ops.bn_relu_pool); on every other path it
materialises the BN+ReLU first and goes on as for a tensor. Either way
the module is called once per pool and returns one tensor."""
import torch.nn as nn


class FusedMaxPool2d(nn.MaxPool2d):
    fused_ops = False  # set by kubeshare_amd.ops.fuse_model

    def forward(self, x):
        from .. import ops
        pending = isinstance(x, ops.PendingBNReLU)
        if self.fused_ops and self.dilation == 1 and not self.ceil_mode \
                and not self.return_indices:
            # KUBESHARE_FUSED_POOL=0: stock path even when flagged
            if ops.fused_pool_enabled():
                # KUBESHARE_BN_POOL=0: BN+ReLU and the pool as two ops
                if pending and ops.bn_pool_enabled():
                    return ops.bn_relu_pool(x.x, x.bn, self.kernel_size,
                                            self.stride, self.padding)
                if pending:
                    x = x.materialize()
                return ops.max_pool_nhwc(x, self.kernel_size, self.stride,
                                         self.padding)
        if pending:
            x = x.materialize()
        return super().forward(x)
