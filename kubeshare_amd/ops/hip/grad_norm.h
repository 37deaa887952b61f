// Layout of the norm workspace shared by grad_norm.hip (which writes it)
// and the clipping / LARS instantiation of the multi-tensor SGD kernel in
// ks_ops.hip (which reads it). One persistent f32 device buffer per
// optimizer, for T tensors whose chunks add up to B blocks:
//
//   [0] norm    sqrt(sum_t sumsq_g[t]), the pre-clip global norm
//   [1] coef    min(1, max_norm / (norm + 1e-6)); 1 without a max_norm
//   [2] finite  1.0f if the total is finite, else 0.0f
//   [3] int32   number of non-finite totals seen so far
//   [4, 4+T)        sumsq_g[t]
//   [4+T, 4+2T)     sumsq_w[t]        (written with LARS only)
//   [4+2T, 4+3T)    sqrt(sumsq_g[t])  (per-tensor norms)
//   [4+3T, +B)      stage-1 partials of the gradients, block order
//   [4+3T+B, +B)    stage-1 partials of the weights (LARS only)
#pragma once

#define KS_NORM_WS_NORM 0
#define KS_NORM_WS_COEF 1
#define KS_NORM_WS_FINITE 2
#define KS_NORM_WS_COUNT 3
#define KS_NORM_WS_HEAD 4

// These kernels are compiled without the packed f32 instructions (a
// device-side feature: the host pass does not know it).
#if defined(__HIP_DEVICE_COMPILE__)
#define KS_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define KS_NO_PK_F32
#endif
