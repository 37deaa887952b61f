// The residual join of a downsample block in one op for gfx950:
//   y = relu(bn(x) + bn_d(x_d))
// with x the block's last conv output and x_d the downsample conv's.
//
// The composition ops.bn_relu(x, bn, res=ops.bn_relu(x_d, bn_d,
// relu=False)) writes the downsample BN's output `id`, reads it straight
// back in the residual apply and keeps it alive until backward; its
// backward writes dres and then reads it twice more in the downsample
// BN's own stats and apply kernels. Nothing else uses either tensor.
// Here `id` stays in registers (rounded to bf16 exactly where the
// composition stored it), and one stats and one apply kernel serve both
// BNs in backward:
//
//   forward   bn_stats + reduce/finalize for each BN (bn_relu.hip's
//             launches, unchanged), then bn_join_apply: reads x, x_d,
//             writes y (+ the ReLU mask byte)
//   backward  bn_join_bwd_stats: reads x, x_d, dy [, dy2], the mask byte
//             (or y); writes dym; block partials of dbias, dscale and
//             dscale_d
//             the two reduce launches of bn_common.h
//             bn_join_bwd_apply: reads x, x_d, dym; writes dx, dx_d
//
// dbias is one sum for both BNs: the composition's downsample BN sums
// the same terms (dres = dym) in the same order.
//
// Layout, row walk (NhwcRows) and block partials are nhwc_common.h's;
// the launch geometry is bn_geom_of's and rows advance grid-stride in
// groups of KS_BN_UNROLL. Every floating-point expression
// goes through a pinned helper of bn_common.h, and each lane keeps its
// rows in the composition's order and in the same groups of four, so
// the results are the composition's bits.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <type_traits>
#include <vector>

#include "bn_common.h"

// Rows loaded per sub-batch in the backward kernels, chosen from the
// compiler's resource report under the 128-VGPR budget (two 512-thread
// blocks per CU); the sweep is in profiles/bn_join_kernels.txt.
#define KS_BN_JOIN_U 2   // stats, two gradients (118 VGPRs; 4: 480 B scratch)
#define KS_BN_JOIN_U1 1  // stats, one gradient (102 VGPRs; 2: 80 B scratch)
#define KS_BN_JOIN_UA 1  // apply (102 VGPRs; 2: 20 B scratch)

// --------------------------------------------------------- fwd apply
template <bool MASK>
__global__ void bn_join_apply_kernel(const ushort8* __restrict__ x,
                                     const ushort8* __restrict__ xd,
                                     ushort8* __restrict__ y,
                                     unsigned char* __restrict__ mask,
                                     const float* __restrict__ scale,
                                     const float* __restrict__ biasf,
                                     const float* __restrict__ scale_d,
                                     const float* __restrict__ biasf_d,
                                     long long M, int CG) {
  const NhwcRows<KS_BN_BLOCK> rows(CG);
  const int cg = rows.cg;
  const long long stride = rows.stride;
  float8 s, b, sd, bd;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    s[j] = scale[cg * 8 + j];
    b[j] = biasf[cg * 8 + j];
    sd[j] = scale_d[cg * 8 + j];
    bd[j] = biasf_d[cg * 8 + j];
  }
  // one element: the downsample branch is rounded to bf16 as
  // bn_apply_relu_kernel<false, false> stored it, then added as
  // bn_apply_relu_kernel<true, true> adds its residual
  auto one = [&](const ushort8& v, const ushort8& vd) {
    ushort8 o;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float id = bf16_to_f32(
          f32_to_bf16(bn_affine(bf16_to_f32(vd[j]), sd[j], bd[j])));
      float f = bn_affine(bf16_to_f32(v[j]), s[j], b[j]);
      f += id;
      o[j] = bn_relu_bf16(f);
    }
    return o;
  };
  long long row = rows.first(M);
  for (; row + (KS_BN_UNROLL - 1) * stride < M;
       row += KS_BN_UNROLL * stride) {
    ushort8 v[KS_BN_UNROLL], vd[KS_BN_UNROLL];
    long long k[KS_BN_UNROLL];
#pragma unroll
    for (int u = 0; u < KS_BN_UNROLL; u++) {
      k[u] = (row + u * stride) * CG + cg;
      v[u] = x[k[u]];
      vd[u] = xd[k[u]];
    }
#pragma unroll
    for (int u = 0; u < KS_BN_UNROLL; u++) {
      const ushort8 o = one(v[u], vd[u]);
      y[k[u]] = o;
      if (MASK) mask[k[u]] = bn_mask_byte(o);
    }
  }
  for (; row < M; row += stride) {
    const long long k = row * CG + cg;
    const ushort8 o = one(x[k], xd[k]);
    y[k] = o;
    if (MASK) mask[k] = bn_mask_byte(o);
  }
}

// --------------------------------------------------------- bwd stats
// g = (y > 0 ? dy [+ dy2] : 0), formed as bn_bwd_stats_kernel forms it;
// dym = bf16(g); dbias = sum g; dscale = sum g * xhat; dscale_d = sum g *
// xhat_d. The composition's downsample BN reads g back from dym, and g
// is a bf16 value already, so both sums see the same terms.
//
// Registers: mean/invstd of two BNs (32) and three accumulator vectors
// (24) stay live across the loop; a sub-batch of U rows adds 16 U
// (two-gradient form) for the loads. Blocks have 512 threads, so 128
// VGPRs keep two blocks per CU. The rows of a group of four are loaded
// KS_BN_JOIN_U (one gradient: KS_BN_JOIN_U1) at a time in a real loop
// (see bn_bwd_stats_kernel); the summation order does not depend on U.
template <bool WITH_DY2, bool MASK>
__global__ void bn_join_bwd_stats_kernel(
    const ushort8* __restrict__ x, const ushort8* __restrict__ xd,
    const ushort8* __restrict__ y, const unsigned char* __restrict__ mask,
    const ushort8* __restrict__ dy, const ushort8* __restrict__ dy2,
    ushort8* __restrict__ dym_out, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ mean_d,
    const float* __restrict__ invstd_d, float* __restrict__ part,
    float* __restrict__ part_d, long long M, int CG) {
  __shared__ float s_red[KS_BN_BLOCK * 8];
  const NhwcRows<KS_BN_BLOCK> rows(CG);
  const int cg = rows.cg;
  const long long stride = rows.stride;
  float8 mu, is, mud, isd;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    mu[j] = mean[cg * 8 + j];
    is[j] = invstd[cg * 8 + j];
    mud[j] = mean_d[cg * 8 + j];
    isd[j] = invstd_d[cg * 8 + j];
  }
  float8 adb = {0, 0, 0, 0, 0, 0, 0, 0};
  float8 ads = {0, 0, 0, 0, 0, 0, 0, 0};
  float8 adsd = {0, 0, 0, 0, 0, 0, 0, 0};
  // one row; `grouped` (std::true_type inside a whole group of four
  // rows) selects bn_acc_dscale's pattern. yv is read only without
  // MASK, mv only with it, g2 only WITH_DY2.
  auto one = [&](auto grouped, long long k, const ushort8& xv,
                 const ushort8& xdv, const ushort8& yv,
                 const unsigned char& mv, const ushort8& gv,
                 const ushort8& g2) {
    constexpr bool G = decltype(grouped)::value;
    ushort8 dm;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float gin =
          WITH_DY2 ? bn_join_grad(gv[j], g2[j]) : bf16_to_f32(gv[j]);
      const bool on = MASK ? ((mv >> j) & 1) != 0 : bf16_to_f32(yv[j]) > 0.f;
      const float g = on ? gin : 0.f;
      adb[j] += g;
      ads[j] = bn_acc_dscale<G>(
          ads[j], g, bn_pool_xhat(bf16_to_f32(xv[j]), mu[j], is[j]), j);
      adsd[j] = bn_acc_dscale<G>(
          adsd[j], g, bn_pool_xhat(bf16_to_f32(xdv[j]), mud[j], isd[j]), j);
      dm[j] = f32_to_bf16(g);
    }
    dym_out[k] = dm;
  };
  constexpr int U = WITH_DY2 ? KS_BN_JOIN_U : KS_BN_JOIN_U1;
  static_assert(KS_BN_UNROLL % U == 0, "sub-batches must tile a group");
  long long row = rows.first(M);
  for (; row + (KS_BN_UNROLL - 1) * stride < M;
       row += KS_BN_UNROLL * stride) {
#pragma unroll 1
    for (int h = 0; h < KS_BN_UNROLL; h += U) {
      ushort8 xv[U], xdv[U], yv[U], gv[U], g2[U];
      unsigned char mv[U];
      long long k[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        k[u] = (row + (h + u) * stride) * CG + cg;
        xv[u] = x[k[u]];
        xdv[u] = xd[k[u]];
        if (MASK) mv[u] = mask[k[u]]; else yv[u] = y[k[u]];
        gv[u] = dy[k[u]];
        if (WITH_DY2) g2[u] = dy2[k[u]];
      }
#pragma unroll
      for (int u = 0; u < U; u++)
        one(std::true_type{}, k[u], xv[u], xdv[u], yv[u], mv[u], gv[u],
            g2[u]);
    }
  }
  for (; row < M; row += stride) {
    const long long k = row * CG + cg;
    const ushort8 xv = x[k], xdv = xd[k], gv = dy[k];
    ushort8 yv, g2;
    unsigned char mv;
    if (MASK) mv = mask[k]; else yv = y[k];
    if (WITH_DY2) g2 = dy2[k];
    one(std::false_type{}, k, xv, xdv, yv, mv, gv, g2);
  }

  // part[0] = dbias, part[1] = dscale, part_d = dscale_d
  const int C = CG * 8;
  nhwc_block_partials<KS_BN_BLOCK>(s_red, adb, part, CG);
  __syncthreads();
  nhwc_block_partials<KS_BN_BLOCK>(s_red, ads,
                                   part + (long long)gridDim.x * C, CG);
  __syncthreads();
  nhwc_block_partials<KS_BN_BLOCK>(s_red, adsd, part_d, CG);
}

// --------------------------------------------------------- bwd apply
// dx   = w'   * (dym - dbias/M - xhat   * dscale/M)
// dx_d = w_d' * (dym - dbias/M - xhat_d * dscale_d/M)
// Nine per-channel vectors stay live (72 VGPRs), so the rows of a group
// are handled KS_BN_JOIN_UA at a time; nothing is summed here, the order
// is free.
__global__ void bn_join_bwd_apply_kernel(
    const ushort8* __restrict__ x, const ushort8* __restrict__ xd,
    const ushort8* __restrict__ dym, ushort8* __restrict__ dx,
    ushort8* __restrict__ dxd, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ weight,
    const float* __restrict__ mean_d, const float* __restrict__ invstd_d,
    const float* __restrict__ weight_d, const float* __restrict__ dbias,
    const float* __restrict__ dscale, const float* __restrict__ dscale_d,
    long long M, int CG) {
  const NhwcRows<KS_BN_BLOCK> rows(CG);
  const int cg = rows.cg;
  const long long stride = rows.stride;
  const float invM = 1.f / (float)M;
  float8 mu, is, w, ds, mud, isd, wd, dsd, db;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int c = cg * 8 + j;
    mu[j] = mean[c];
    is[j] = invstd[c];
    w[j] = weight[c] * is[j];
    ds[j] = dscale[c] * invM;
    mud[j] = mean_d[c];
    isd[j] = invstd_d[c];
    wd[j] = weight_d[c] * isd[j];
    dsd[j] = dscale_d[c] * invM;
    db[j] = dbias[c] * invM;
  }
  auto one = [&](long long k, const ushort8& xv, const ushort8& xdv,
                 const ushort8& gv) {
    ushort8 o, od;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float g = bf16_to_f32(gv[j]);  // already ReLU-masked
      o[j] = f32_to_bf16(bn_pool_dx(
          w[j], g, db[j], bn_pool_xhat(bf16_to_f32(xv[j]), mu[j], is[j]),
          ds[j]));
      od[j] = f32_to_bf16(bn_pool_dx(
          wd[j], g, db[j],
          bn_pool_xhat(bf16_to_f32(xdv[j]), mud[j], isd[j]), dsd[j]));
    }
    dx[k] = o;
    dxd[k] = od;
  };
  constexpr int U = KS_BN_JOIN_UA;
  long long row = rows.first(M);
  for (; row + (U - 1) * stride < M; row += U * stride) {
    ushort8 xv[U], xdv[U], gv[U];
    long long k[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      k[u] = (row + u * stride) * CG + cg;
      xv[u] = x[k[u]];
      xdv[u] = xd[k[u]];
      gv[u] = dym[k[u]];
    }
#pragma unroll
    for (int u = 0; u < U; u++) one(k[u], xv[u], xdv[u], gv[u]);
  }
  for (; row < M; row += stride) {
    const long long k = row * CG + cg;
    const ushort8 xv = x[k], xdv = xd[k], gv = dym[k];
    one(k, xv, xdv, gv);
  }
}

// ================================================================== host
namespace {

void check_pair(const torch::Tensor& x, const torch::Tensor& x_d,
                const char* what) {
  TORCH_CHECK(x_d.is_cuda() && x_d.sizes() == x.sizes() &&
                  x_d.scalar_type() == at::kBFloat16 &&
                  x_d.is_contiguous(at::MemoryFormat::ChannelsLast),
              what, ": x_d must be channels-last bf16 of x's shape");
}

}  // namespace

std::vector<torch::Tensor> bn_join_fwd_train(
    torch::Tensor x, torch::Tensor weight, torch::Tensor bias,
    torch::Tensor running_mean, torch::Tensor running_var, double momentum,
    double eps, torch::Tensor x_d, torch::Tensor weight_d,
    torch::Tensor bias_d, torch::Tensor running_mean_d,
    torch::Tensor running_var_d, double momentum_d, double eps_d,
    bool want_mask, bool legacy_reduce) {
  BnGeom g = bn_geom_of(x);
  check_pair(x, x_d, "bn_join_fwd_train");
  auto stream = at::cuda::getCurrentCUDAStream();
  auto f32 = x.options().dtype(at::kFloat);
  auto y = at::empty_like(x);
  auto mean = at::empty({g.C}, f32), invstd = at::empty({g.C}, f32);
  auto mean_d = at::empty({g.C}, f32), invstd_d = at::empty({g.C}, f32);
  auto scale = at::empty({g.C}, f32), biasf = at::empty({g.C}, f32);
  auto scale_d = at::empty({g.C}, f32), biasf_d = at::empty({g.C}, f32);
  auto fptr = [](torch::Tensor& t) {
    return t.defined() ? t.data_ptr<float>() : nullptr;
  };
  // the composition's own statistics launches, downsample BN first
  bn_launch_fwd_stats(x_d, g, weight_d, bias_d, fptr(running_mean_d),
                      fptr(running_var_d), mean_d, invstd_d, scale_d, biasf_d,
                      momentum_d, eps_d, legacy_reduce, stream.stream());
  bn_launch_fwd_stats(x, g, weight, bias, fptr(running_mean),
                      fptr(running_var), mean, invstd, scale, biasf, momentum,
                      eps, legacy_reduce, stream.stream());
  torch::Tensor mask;
  if (want_mask)
    mask = at::empty({x.size(0), x.size(2), x.size(3), (long long)g.CG},
                     x.options().dtype(at::kByte));
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(g.blocks), dim3(KS_BN_BLOCK), 0,
                       stream.stream(), nhwc_cptr(x), nhwc_cptr(x_d),
                       nhwc_mptr(y),
                       want_mask ? mask.data_ptr<unsigned char>() : nullptr,
                       scale.data_ptr<float>(), biasf.data_ptr<float>(),
                       scale_d.data_ptr<float>(), biasf_d.data_ptr<float>(),
                       g.M, g.CG);
  };
  want_mask ? launch(bn_join_apply_kernel<true>)
            : launch(bn_join_apply_kernel<false>);
  if (want_mask) return {y, mean, invstd, mean_d, invstd_d, mask};
  return {y, mean, invstd, mean_d, invstd_d};
}

std::vector<torch::Tensor> bn_join_bwd(
    torch::Tensor x, torch::Tensor x_d, torch::Tensor y_or_mask,
    torch::Tensor dy, c10::optional<torch::Tensor> dy2, torch::Tensor weight,
    torch::Tensor weight_d, torch::Tensor mean, torch::Tensor invstd,
    torch::Tensor mean_d, torch::Tensor invstd_d, bool use_mask,
    bool legacy_reduce) {
  BnGeom g = bn_geom_of(x);
  check_pair(x, x_d, "bn_join_bwd");
  TORCH_CHECK(dy.sizes() == x.sizes() && dy.scalar_type() == at::kBFloat16,
              "bn_join_bwd: dy must be bf16 of x's shape");
  if (use_mask)
    bn_check_mask(y_or_mask, x, g);
  else
    check_pair(x, y_or_mask, "bn_join_bwd (y)");
  // second upstream gradient: as in bn_relu_bwd
  bool fold_dy2 = false;
  if (dy2.has_value() && dy2->defined()) {
    TORCH_CHECK(dy2->sizes() == x.sizes(),
                "bn_join_bwd: dy2 must have x's shape");
    fold_dy2 = dy2->is_cuda() && dy2->scalar_type() == at::kBFloat16 &&
               dy2->is_contiguous(at::MemoryFormat::ChannelsLast) &&
               dy.is_contiguous(at::MemoryFormat::ChannelsLast);
    if (!fold_dy2) dy = (dy + *dy2).to(at::kBFloat16);
  }
  if (!dy.is_contiguous(at::MemoryFormat::ChannelsLast))
    dy = dy.contiguous(at::MemoryFormat::ChannelsLast);
  auto stream = at::cuda::getCurrentCUDAStream();
  auto f32 = x.options().dtype(at::kFloat);
  // part: dbias and dscale halves, then the dscale_d partials
  auto part = at::empty({(long long)3 * g.stat_blocks * g.C}, f32);
  float* part_p = part.data_ptr<float>();
  float* part_d_p = part_p + (long long)2 * g.stat_blocks * g.C;
  auto red = at::empty({g.C * 3}, f32);
  float* dbias_p = red.data_ptr<float>();
  float* dscale_p = dbias_p + g.C;
  float* dscale_d_p = dscale_p + g.C;
  auto dym = at::empty_like(x);  // scratch: freed on return
  auto dx = at::empty_like(x);
  auto dx_d = at::empty_like(x);
  auto launch_stats = [&](auto kern) {
    hipLaunchKernelGGL(
        kern, dim3(g.stat_blocks), dim3(KS_BN_BLOCK), 0, stream.stream(),
        nhwc_cptr(x), nhwc_cptr(x_d), use_mask ? nullptr : nhwc_cptr(y_or_mask),
        use_mask ? y_or_mask.data_ptr<unsigned char>() : nullptr, nhwc_cptr(dy),
        fold_dy2 ? nhwc_cptr(*dy2) : nullptr, nhwc_mptr(dym),
        mean.data_ptr<float>(),
        invstd.data_ptr<float>(), mean_d.data_ptr<float>(),
        invstd_d.data_ptr<float>(), part_p, part_d_p, g.M, g.CG);
  };
  if (use_mask)
    fold_dy2 ? launch_stats(bn_join_bwd_stats_kernel<true, true>)
             : launch_stats(bn_join_bwd_stats_kernel<false, true>);
  else
    fold_dy2 ? launch_stats(bn_join_bwd_stats_kernel<true, false>)
             : launch_stats(bn_join_bwd_stats_kernel<false, false>);
  bn_launch_bwd_reduce(part_p, g.stat_blocks, g.C, dbias_p, dscale_p,
                       legacy_reduce, stream.stream());
  bn_launch_reduce_one(part_d_p, g.stat_blocks, g.C, dscale_d_p,
                       stream.stream());
  hipLaunchKernelGGL(bn_join_bwd_apply_kernel, dim3(g.blocks),
                     dim3(KS_BN_BLOCK), 0, stream.stream(), nhwc_cptr(x),
                     nhwc_cptr(x_d), nhwc_cptr(dym), nhwc_mptr(dx),
                     nhwc_mptr(dx_d),
                     mean.data_ptr<float>(), invstd.data_ptr<float>(),
                     weight.data_ptr<float>(), mean_d.data_ptr<float>(),
                     invstd_d.data_ptr<float>(), weight_d.data_ptr<float>(),
                     dbias_p, dscale_p, dscale_d_p, g.M, g.CG);
  return {dx, dx_d, red.narrow(0, g.C, g.C), red.narrow(0, 0, g.C),
          red.narrow(0, 2 * g.C, g.C)};
}
