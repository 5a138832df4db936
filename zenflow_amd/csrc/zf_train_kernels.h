// The trainer's element-wise kernels: ShiftBounds, BatchNorm with batch
// statistics (multi-launch and single-block), gather / scatter of the
// conditioner's inputs, the eval-mode vector-Jacobian kernels, latent
// log-density and loss, the gradient cast and the (n)adamw update.
#pragma once
#include "zf_internal.h"
#include "zf_reduce.h"

#include <cmath>

namespace zf {
namespace {

constexpr float kBnEps = 1e-5f;     // flax.linen.BatchNorm epsilon
constexpr float kBnMomentum = 0.99f; // flax.linen.BatchNorm momentum

// ---- ShiftBounds (train mode; bijectors.py:163-273) -------------------------
// Natural row per dim: [mode, a, b, xmin, xmax, margin, -, -].  Batch min/max
// of the (safe_log-transformed) column -> running xmin/xmax (:250-259).
// This batch's min / max widened by the margin and merged with the running
// values, then the affine map, clip and log-det.  Every thread forms the
// statistics from the column min / max itself (a handful of scalars: no
// separate statistics launch); thread 0 also writes the running values when
// update is set — the one write another block can observe, and re-forming
// the statistics from it gives the same values (min / max are idempotent).
// first: this op starts the chain, so ld (not yet written this step) is set
// instead of accumulated.
__global__ void sb_forward_kernel(const float* __restrict__ x, float* __restrict__ y, float* __restrict__ ld,
                                  float* __restrict__ sb, int B, int D, int rot, const float* __restrict__ cmin,
                                  const float* __restrict__ cmax, int update, int first) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float lds = 0.f;
  for (int i = 0; i < D; ++i) {
    const int p = pmodi(i + rot, D);
    const float v = x[(long long)b * D + p];
    float* r = sb + 8 * i;
    const int mode = (int)r[0];
    const float a = r[1], bb = r[2];
    float z, l;
    if (mode == ZF_SB_BOTH) {
      const float mul = (float)(1.0 / ((double)bb - (double)a));
      z = (v - a) * mul;
      l = logf(mul);
    } else {
      const float margin = r[5];
      float xmin = cmin[i], xmax = cmax[i];
      const float delta = 0.5f * (xmax - xmin) * margin;
      xmin = xmin - delta;
      xmax = xmax + delta;
      xmin = fminf(r[3], xmin);  // jnp.minimum(ra_min, xmin); NaN from the batch propagates below
      xmax = fmaxf(r[4], xmax);
      if (cmin[i] != cmin[i]) xmin = cmin[i];
      if (cmax[i] != cmax[i]) xmax = cmax[i];
      if (update && b == 0) {
        r[3] = xmin;
        r[4] = xmax;
      }
      const float mul = 1.0f / (xmax - xmin);
      float t = v;
      if (mode == ZF_SB_LOWER) t = logf((v - a) + 1.17549435e-38f);
      if (mode == ZF_SB_UPPER) t = logf((bb - v) + 1.17549435e-38f);
      const float zr = (t - xmin) * mul;
      z = (zr != zr) ? zr : fminf(fmaxf(zr, 0.f), 1.f);
      l = (mode == ZF_SB_NONE) ? logf(mul) : logf(mul) - t;
    }
    lds = lds + l;
    y[(long long)b * D + p] = z;
  }
  ld[b] = (first ? 0.f : ld[b]) + lds;
}

// ---- NeuralSplineCoupling pieces --------------------------------------------
// U = hstack(xc, c): logical conditioning dim k is column pmod(dt + k + rot, D).
__global__ void gather_u_kernel(const float* __restrict__ s, const float* __restrict__ c, float* __restrict__ U,
                                int B, int D, int C, int dt, int dc, int rot) {
  const int DC = dc + C;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)B * DC) return;
  const long long b = i / DC;
  const int k = (int)(i - b * DC);
  U[i] = k < dc ? s[b * D + pmodi(dt + k + rot, D)] : c[b * C + (k - dc)];
}

// BatchNorm with batch statistics (flax, use_running_average=False):
// mean, var = max(0, E[u^2] - E[u]^2); u_hat = (u - mean) * rsqrt(var + eps);
// u_bn = u_hat * scale + bias.  Also the running-average update (momentum 0.99).
// sum / sumsq: fp64 column sums over the global batch of Bg rows.
__device__ __forceinline__ void bn_stats_one(double sum, double sumsq, long long Bg, int k, int DC,
                                             float* __restrict__ nat_bn, float& mean, float& rstd, int update) {
#pragma clang fp contract(off)
  // every operation separately rounded: the same bits in every kernel that inlines this
  const double md = sum / Bg;
  mean = (float)md;
  const float mean2 = (float)(sumsq / Bg);
  float var = fmaxf(0.f, mean2 - mean * mean);  // flax's form, on fp32 moments
  // That difference is off by ulp(mean2) / var of itself, 2^-24 mean2 / var.
  // From mean2 / var = 256 on (a column that varies by under 6% of its level:
  // a batch of two or three rows, a near-constant condition) that is 1.5e-5
  // and more, past the 1e-5 every gradient is held to: 6e-4 for a column at
  // 0.38 whose two rows differ by 0.01 reached the gradient at 2.5e-4 of scale
  // (test_train_gradient_per_parameter[small-2-86]).  There the difference of
  // the fp64 moments, rounded once, takes its place.  Better-conditioned
  // columns keep the fp32 form and with it the bits they always had.
  if (var * 256.f < mean2) var = fmaxf(0.f, (float)(sumsq / Bg - md * md));
  rstd = 1.0f / sqrtf(var + kBnEps);
  if (update) {
    nat_bn[k] = kBnMomentum * nat_bn[k] + (1.0f - kBnMomentum) * mean;
    nat_bn[DC + k] = kBnMomentum * nat_bn[DC + k] + (1.0f - kBnMomentum) * var;
  }
}

__global__ void bn_stats_kernel(const double* __restrict__ csum, const double* __restrict__ csq, long long Bg, int DC,
                                float* __restrict__ nat_bn, float* __restrict__ mean_out,
                                float* __restrict__ rstd_out, int update) {
  const int k = threadIdx.x;
  if (k >= DC) return;
  float mean, rstd;
  bn_stats_one(csum[k], csq[k], Bg, k, DC, nat_bn, mean, rstd, update);
  mean_out[k] = mean;
  rstd_out[k] = rstd;
}

// Per-element BatchNorm arithmetic shared by the single-block and the
// multi-launch paths, every operation separately rounded (fp contraction off:
// HIP's __f*_rn are plain operators that the compiler may still fuse, and it
// fuses differently in different kernels): both paths give the same bits.
__device__ __forceinline__ float bn_hat(float u, float mean, float rstd) {
#pragma clang fp contract(off)
  return (u - mean) * rstd;
}
__device__ __forceinline__ float bn_out(float uh, float scale, float bias) {
#pragma clang fp contract(off)
  return uh * scale + bias;
}
// reverse: the mean terms scale * sum / Bg, then
// dL/dU = rstd * (gUbn * scale - mg - Uhat * mgu)
__device__ __forceinline__ float bn_mean_term(float scale, double sum, long long Bg) {
#pragma clang fp contract(off)
  return scale * (float)sum / (float)Bg;
}
__device__ __forceinline__ float bn_grad_in(float gubn, float uh, float scale, float rstd, float mg, float mgu) {
#pragma clang fp contract(off)
  return rstd * (gubn * scale - mg - uh * mgu);
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

__global__ void bn_apply_kernel(const float* __restrict__ U, const float* __restrict__ mean,
                                const float* __restrict__ rstd, const float* __restrict__ scale,
                                const float* __restrict__ bias, float* __restrict__ Uhat, float* __restrict__ Ubn,
                                int B, int DC) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)B * DC) return;
  const int k = (int)(i % DC);
  const float uh = bn_hat(U[i], mean[k], rstd[k]);
  Uhat[i] = uh;
  Ubn[i] = bn_out(uh, scale[k], bias[k]);
}

}  // namespace
}  // namespace zf

// The spline rows, here and not at the top: a code object holds its kernels in
// the order of their definitions, and spline_inv_kernel stood between the
// forward and the reverse BatchNorm kernels when all this was one file.  The
// trainer's code object is held to those bytes (Training).
#include "zf_train_spline.h"

namespace zf {
namespace {

// BatchNorm reverse with batch statistics:
// gU = rstd * (gUhat - mean(gUhat) - u_hat * mean(gUhat * u_hat)), gUhat = gUbn * scale.
__global__ void bn_bwd_kernel(const float* __restrict__ gUbn, const float* __restrict__ Uhat,
                              const float* __restrict__ scale, const float* __restrict__ rstd,
                              const double* __restrict__ sum_g, const double* __restrict__ sum_gu,
                              float* __restrict__ gU, int B, long long Bg, int DC) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)B * DC) return;
  const int k = (int)(i % DC);
  // sum_g / sum_gu: global sums of gUbn and gUbn*Uhat; scaled into gUhat terms
  const float mg = bn_mean_term(scale[k], sum_g[k], Bg), mgu = bn_mean_term(scale[k], sum_gu[k], Bg);
  gU[i] = bn_grad_in(gUbn[i], Uhat[i], scale[k], rstd[k], mg, mgu);
}

// ---- small batches: BatchNorm forward / reverse in one single-block launch --
// (B * DC <= kBnSmall, one device).  The same arithmetic as the multi-launch
// path (gather_u + leaf_colsums + tree + bn_stats + bn_apply forward;
// leaf_colsums + tree + bn_bwd + scatter reverse): the same leaf_sums2 per
// (leaf, column) and the same tree_n over the leaves, here through LDS.
constexpr long long kBnSmall = 1ll << 14;
constexpr int kBnLeafCap = kLeafCap;  // leaves of a BatchNorm sum (both paths)

__global__ __launch_bounds__(1024) void bn_fwd_small(const float* __restrict__ s, const float* __restrict__ c,
                                                     float* __restrict__ Uhat, float* __restrict__ Ubn,
                                                     float* __restrict__ nat_bn, float* __restrict__ mean_out,
                                                     float* __restrict__ rstd_out, int B, int D, int C, int dt, int dc,
                                                     int rot, int n, int rows, int update) {
  __shared__ double p1[kMaxLeaves * 64], p2[kMaxLeaves * 64];
  __shared__ float smean[64], srstd[64];
  const int DC = dc + C, tid = threadIdx.x;
  auto u_at = [&](long long b, int kk) { return kk < dc ? s[b * D + pmodi(dt + kk + rot, D)] : c[b * C + (kk - dc)]; };
  for (int t = tid; t < n * DC; t += 1024) {
    const int z = t / DC, k = t - z * DC;
    const int b0 = min(B, z * rows), b1 = min(B, b0 + rows);
    leaf_sums2([&](int b) { return u_at(b, k); }, [&](int b) { return u_at(b, k); }, b0, b1, p1[t], p2[t]);
  }
  __syncthreads();
  lds_tree2(p1, p2, n, DC, DC);
  if (tid < DC) {
    float mean, rstd;
    bn_stats_one(p1[tid], p2[tid], B, tid, DC, nat_bn, mean, rstd, update);
    smean[tid] = mean;
    srstd[tid] = rstd;
    mean_out[tid] = mean;
    rstd_out[tid] = rstd;
  }
  __syncthreads();
  const float* scale = nat_bn + 2 * DC;
  const float* bias = nat_bn + 3 * DC;
  for (long long i = tid; i < (long long)B * DC; i += 1024) {
    const long long b = i / DC;
    const int kk = (int)(i - b * DC);
    const float uh = bn_hat(u_at(b, kk), smean[kk], srstd[kk]);
    Uhat[i] = uh;
    Ubn[i] = bn_out(uh, scale[kk], bias[kk]);
  }
}

// gUbn = dL/dUbn -> BatchNorm scale / bias gradients (fp64 accumulator) and
// dL/dU; the conditioning columns' share is added to g (dL/d state) in place.
__global__ __launch_bounds__(1024) void bn_bwd_small(const float* __restrict__ gUbn, const float* __restrict__ Uhat,
                                                     const float* __restrict__ scale, const float* __restrict__ rstd,
                                                     double* __restrict__ g_scale, double* __restrict__ g_bias,
                                                     float* __restrict__ g, int B, int D, int C, int dt, int dc,
                                                     int rot, int n, int rows, float* __restrict__ gc = nullptr,
                                                     int gc_assign = 0) {
  __shared__ double p1[kMaxLeaves * 64], p2[kMaxLeaves * 64];
  __shared__ float mg_s[64], mgu_s[64];
  const int DC = dc + C, tid = threadIdx.x;
  for (int t = tid; t < n * DC; t += 1024) {
    const int z = t / DC, k = t - z * DC;
    const int b0 = min(B, z * rows), b1 = min(B, b0 + rows);
    leaf_sums2([&](int b) { return gUbn[(long long)b * DC + k]; }, [&](int b) { return Uhat[(long long)b * DC + k]; },
               b0, b1, p1[t], p2[t]);
  }
  __syncthreads();
  lds_tree2(p1, p2, n, DC, DC);
  if (tid < DC) {
    const double sg = p1[tid], sgu = p2[tid];
    g_scale[tid] = sgu;
    g_bias[tid] = sg;
    mg_s[tid] = bn_mean_term(scale[tid], sg, B);
    mgu_s[tid] = bn_mean_term(scale[tid], sgu, B);
  }
  __syncthreads();
  for (long long i = tid; i < (long long)B * dc; i += 1024) {
    const long long b = i / dc;
    const int kk = (int)(i - b * dc);
    const long long e = b * DC + kk;
    const float gu = bn_grad_in(gUbn[e], Uhat[e], scale[kk], rstd[kk], mg_s[kk], mgu_s[kk]);
    // a separately rounded add (no fma with the product above), as the
    // multi-launch path's scatter_gu_kernel adds a stored gU
    float* gp = g + b * D + pmodi(dt + kk + rot, D);
    *gp = add_rn(*gp, gu);
  }
  // the condition columns' share, d loss / d c (gather_gc_kernel's arithmetic)
  if (gc) {
    for (long long i = tid; i < (long long)B * C; i += 1024) {
      const long long b = i / C;
      const int kk = dc + (int)(i - b * C);
      const long long e = b * DC + kk;
      const float gu = bn_grad_in(gUbn[e], Uhat[e], scale[kk], rstd[kk], mg_s[kk], mgu_s[kk]);
      gc[i] = gc_assign ? gu : add_rn(gc[i], gu);
    }
  }
}

__global__ void scatter_gu_kernel(const float* __restrict__ gU, float* __restrict__ g, int B, int D, int C, int dt,
                                  int dc, int rot) {
  const int DC = dc + C;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)B * dc) return;
  const long long b = i / dc;
  const int k = (int)(i - b * dc);
  float* gp = g + b * D + pmodi(dt + k + rot, D);
  *gp = add_rn(*gp, gU[b * DC + k]);
}

// The condition columns of gU = d loss / d U (columns dc .. dc + C) into
// gc = d loss / d c: the coupling nearest the latent assigns, the ones before
// it add in a fixed order (the reverse loop's), each add separately rounded.
__global__ void gather_gc_kernel(const float* __restrict__ gU, float* __restrict__ gc, int B, int C, int dc,
                                 int assign) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)B * C) return;
  const long long b = i / C;
  const float gu = gU[b * (dc + C) + dc + (int)(i - b * C)];
  gc[i] = assign ? gu : add_rn(gc[i], gu);
}

// ---- eval-mode vector-Jacobian product of log_prob (flow.py:22-48) ----------
// The same op-by-op chain with the stored statistics (BatchNorm mean / var,
// ShiftBounds xmin / xmax): every row is independent, so there are no batch
// reductions; the reverse pass carries a per-row cotangent ce = d (sum cot lp)
// / d lp_row, zeroed on rows whose log_prob is not finite (the `where`
// gradient of flow.py:47's nan_to_num), and yields d / d x and d / d c.

// ShiftBounds with the stored xmin / xmax (bijectors.py:258-273, train=False),
// first op of the chain (rot == 0): sets ld.
__global__ void sb_eval_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, float* __restrict__ ld,
                                   const float* __restrict__ sb, int B, int D) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float lds = 0.f;
  for (int i = 0; i < D; ++i) {
    const float v = x[(long long)b * D + i];
    const float* r = sb + 8 * i;
    const int mode = (int)r[0];
    const float a = r[1], bb = r[2];
    float z, l;
    if (mode == ZF_SB_BOTH) {
      const float mul = (float)(1.0 / ((double)bb - (double)a));
      z = (v - a) * mul;
      l = logf(mul);
    } else {
      const float xmin = r[3], xmax = r[4];
      const float mul = 1.0f / (xmax - xmin);
      float t = v;
      if (mode == ZF_SB_LOWER) t = logf((v - a) + 1.17549435e-38f);
      if (mode == ZF_SB_UPPER) t = logf((bb - v) + 1.17549435e-38f);
      const float zr = (t - xmin) * mul;
      z = (zr != zr) ? zr : fminf(fmaxf(zr, 0.f), 1.f);
      l = (mode == ZF_SB_NONE) ? logf(mul) : logf(mul) - t;
    }
    lds = lds + l;
    y[(long long)b * D + i] = z;
  }
  ld[b] = lds;
}

// Its reverse and the end of the chain's reverse pass: gx = g . dz/dx +
// ce . d log_det / dx per dim (sb == NULL: no ShiftBounds, gx = g).
//   BOTH  z = (x - a) mul                      -> g mul
//   NONE  z = clip((x - xmin) mul, 0, 1)        -> g mul inside (0, 1), else 0
//   LOWER / UPPER the same through t = safe_log(+-(x - a)), dt/dx =
//         +-1 / (+-(x - a) + tiny), and log_det = log(mul) - t -> (.. - ce) dt/dx
// A row with ce == 0 (log_prob not finite, or a zero cotangent) is written as
// zeros whatever its intermediates hold.
__global__ void sb_eval_bwd_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                   const float* __restrict__ ce, const float* __restrict__ sb,
                                   float* __restrict__ gx, int B, int D) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)B * D) return;
  const long long b = e / D;
  const int i = (int)(e - b * D);
  const float cb = ce[b];
  float out = g[e];
  if (sb) {
    const float* r = sb + 8 * i;
    const int mode = (int)r[0];
    const float a = r[1], bb = r[2], v = x[e];
    if (mode == ZF_SB_BOTH) {
      out = out * (float)(1.0 / ((double)bb - (double)a));
    } else {
      const float xmin = r[3], xmax = r[4];
      const float mul = 1.0f / (xmax - xmin);
      float t = v, dtdx = 1.0f;
      if (mode == ZF_SB_LOWER) {
        const float w = (v - a) + 1.17549435e-38f;
        t = logf(w);
        dtdx = 1.0f / w;
      }
      if (mode == ZF_SB_UPPER) {
        const float w = (bb - v) + 1.17549435e-38f;
        t = logf(w);
        dtdx = -1.0f / w;
      }
      const float zr = (t - xmin) * mul;
      float gt = (zr > 0.f && zr < 1.f) ? out * mul : 0.f;
      if (mode != ZF_SB_NONE) gt = gt - cb;
      out = gt * dtdx;
    }
  }
  gx[e] = cb == 0.f ? 0.f : out;
}

// U = hstack(xc, c) and BatchNorm with the stored statistics (flax,
// use_running_average=True): Ubn = (u - mean) rsqrt(var + eps) scale + bias.
// Row 0's threads also store rstd[k] = rsqrt(var + eps), all the reverse needs.
__global__ void bn_eval_fwd_kernel(const float* __restrict__ s, const float* __restrict__ c,
                                   const float* __restrict__ nat_bn, float* __restrict__ Ubn,
                                   float* __restrict__ rstd_out, int B, int D, int C, int dt, int dc, int rot) {
  const int DC = dc + C;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)B * DC) return;
  const long long b = i / DC;
  const int k = (int)(i - b * DC);
  const float u = k < dc ? s[b * D + pmodi(dt + k + rot, D)] : c[b * C + (k - dc)];
  const float rstd = 1.0f / sqrtf(nat_bn[DC + k] + kBnEps);
  if (b == 0) rstd_out[k] = rstd;
  Ubn[i] = bn_out(bn_hat(u, nat_bn[k], rstd), nat_bn[2 * DC + k], nat_bn[3 * DC + k]);
}

// Its reverse, gU = gUbn scale rstd, with the scatter fused: the dc state
// columns are added into g (d / d state, as scatter_gu_kernel), the C
// condition columns assigned to / added into gc (as gather_gc_kernel; gc may
// be NULL).  Rows with ce == 0 contribute exact zeros.
__global__ void bn_eval_bwd_kernel(const float* __restrict__ gUbn, const float* __restrict__ scale,
                                   const float* __restrict__ rstd, const float* __restrict__ ce,
                                   float* __restrict__ g, float* __restrict__ gc, int gc_assign, int B, int D, int C,
                                   int dt, int dc, int rot) {
#pragma clang fp contract(off)
  const int DC = dc + C;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)B * DC) return;
  const long long b = i / DC;
  const int k = (int)(i - b * DC);
  const float gu = ce[b] == 0.f ? 0.f : (gUbn[i] * scale[k]) * rstd[k];
  if (k < dc) {
    float* gp = g + b * D + pmodi(dt + k + rot, D);
    *gp = *gp + gu;
  } else if (gc) {
    float* gp = gc + b * C + (k - dc);
    *gp = gc_assign ? gu : *gp + gu;
  }
}

// Latent log-density with a per-row cotangent (cot NULL: ones): lp_out =
// nan_to_num(latent.log_prob(z) + ld) (flow.py:45-47; NULL: not wanted), ce =
// cot where that sum is finite and 0 elsewhere, gz = ce . d latent_lp / dz —
// latent_loss_kernel's densities and `fin` rule, the rule applied to the
// log-det cotangent ce as well.
__global__ __launch_bounds__(256) void latent_vjp_kernel(const float* __restrict__ z, const float* __restrict__ ld,
                                                         const float* __restrict__ cot, int B, int D, int rot,
                                                         int latent, float a, float betac, float tnmass,
                                                         float* __restrict__ lp_out, float* __restrict__ ce,
                                                         float* __restrict__ gz) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float lat = 0.f;
  for (int j = 0; j < D; ++j) {
    const float v = z[(long long)b * D + pmodi(j + rot, D)];
    float t;
    if (latent == ZF_LATENT_NORMAL || latent == ZF_LATENT_TRUNCNORM) {
      const float dv = v - 0.5f;
      t = (logf(6.28318530717958647692f * 0.01f) + (dv * dv) / 0.01f) / -2.0f;
      if (latent == ZF_LATENT_TRUNCNORM) {
        t = t - tnmass;
        if (dv / 0.1f < -5.f || dv / 0.1f > 5.f) t = -INFINITY;
      }
    } else if (latent == ZF_LATENT_BETA) {
      const float am1 = a - 1.0f;
      t = betac + (am1 == 0.f ? 0.f : am1 * logf(v)) + (am1 == 0.f ? 0.f : am1 * log1pf(-v));
      if (v > 1.f || v < 0.f) t = -INFINITY;
    } else if (latent == ZF_LATENT_UNIFORM) {
      t = (v > 1.f || v < 0.f) ? -INFINITY : 0.f;
    } else {
      t = 0.f;
    }
    lat = lat + t;
  }
  float lp = lat + ld[b];
  const bool fin = (lp == lp) && lp != INFINITY && lp != -INFINITY;
  if (lp != lp) lp = -INFINITY;
  if (lp == INFINITY) lp = 3.40282347e38f;
  if (lp == -INFINITY) lp = -3.40282347e38f;
  if (lp_out) lp_out[b] = lp;
  const float s = fin ? (cot ? cot[b] : 1.0f) : 0.f;
  ce[b] = s;
  for (int j = 0; j < D; ++j) {
    const int col = pmodi(j + rot, D);
    const float v = z[(long long)b * D + col];
    float g = 0.f;
    if (s != 0.f) {
      if (latent == ZF_LATENT_NORMAL || latent == ZF_LATENT_TRUNCNORM) g = -(v - 0.5f) / 0.01f;
      else if (latent == ZF_LATENT_BETA) g = (a - 1.0f) / v - (a - 1.0f) / (1.0f - v);
    }
    gz[(long long)b * D + col] = s * g;
  }
}

// ---- latent + loss ------------------------------------------------------------
// lp = latent.log_prob(z) + log_det, nan_to_num (flow.py:45-47); per-row
// loss terms -lp/Bg (fp64, summed by the leaf tree); gz = -(1/Bg) d latent_lp
// / dz (zero where lp is not finite).  Bg: the global batch size.
// leaf_rows > 0 (a divisor of the 256-row block): the block also forms the
// loss leaf sums of its rows in row order, as leaf_sum_kernel does, into
// leaf[block's leaves], the last block zeroing leaves past the last row
// (one launch fewer per step).
__global__ __launch_bounds__(256) void latent_loss_kernel(const float* __restrict__ z, const float* __restrict__ ld,
                                                          int B, long long Bg, int D, int rot, int latent, float a,
                                                          float betac, float tnmass, float* __restrict__ gz,
                                                          double* __restrict__ row_loss, int leaf_rows,
                                                          int leaf_n, double* __restrict__ leaf) {
  __shared__ double rl[256];
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) {
    float lat = 0.f;
    for (int j = 0; j < D; ++j) {
      const float v = z[(long long)b * D + pmodi(j + rot, D)];
      float t;
      if (latent == ZF_LATENT_NORMAL || latent == ZF_LATENT_TRUNCNORM) {
        const float dv = v - 0.5f;
        t = (logf(6.28318530717958647692f * 0.01f) + (dv * dv) / 0.01f) / -2.0f;
        if (latent == ZF_LATENT_TRUNCNORM) {
          t = t - tnmass;
          if (dv / 0.1f < -5.f || dv / 0.1f > 5.f) t = -INFINITY;
        }
      } else if (latent == ZF_LATENT_BETA) {
        const float am1 = a - 1.0f;
        t = betac + (am1 == 0.f ? 0.f : am1 * logf(v)) + (am1 == 0.f ? 0.f : am1 * log1pf(-v));
        if (v > 1.f || v < 0.f) t = -INFINITY;
      } else {
        t = (v > 1.f || v < 0.f) ? -INFINITY : 0.f;
      }
      lat = lat + t;
    }
    float lp = lat + ld[b];
    const bool fin = (lp == lp) && lp != INFINITY && lp != -INFINITY;
    if (lp != lp) lp = -INFINITY;
    if (lp == INFINITY) lp = 3.40282347e38f;
    if (lp == -INFINITY) lp = -3.40282347e38f;
    row_loss[b] = -(double)lp / (double)Bg;
    const float s = -1.0f / (float)Bg;
    for (int j = 0; j < D; ++j) {
      const int col = pmodi(j + rot, D);
      const float v = z[(long long)b * D + col];
      float g = 0.f;
      if (fin) {
        if (latent == ZF_LATENT_NORMAL || latent == ZF_LATENT_TRUNCNORM) g = -(v - 0.5f) / 0.01f;
        else if (latent == ZF_LATENT_BETA) g = (a - 1.0f) / v - (a - 1.0f) / (1.0f - v);
      }
      gz[(long long)b * D + col] = s * g;
    }
    rl[threadIdx.x] = -(double)lp / (double)Bg;
  }
  if (leaf_rows <= 0) return;
  __syncthreads();
  const int per = 256 / leaf_rows, z0 = blockIdx.x * 256;
  if ((int)threadIdx.x < per) {
    const int r0 = z0 + threadIdx.x * leaf_rows;
    if (r0 < B) {
      const int r1 = min(B, r0 + leaf_rows);
      double acc = 0.0;
      for (int r = r0; r < r1; ++r) acc += rl[r - z0];
      leaf[r0 / leaf_rows] = acc;
    }
  }
  if (blockIdx.x == gridDim.x - 1)  // the leaves past the last row are empty (0, as leaf_sum_kernel)
    for (int zl = (B + leaf_rows - 1) / leaf_rows + (int)threadIdx.x; zl < leaf_n; zl += 256) leaf[zl] = 0.0;
}

// ---- weighted latent + loss --------------------------------------------------
// loss = -sum_b w_b lp_b / Wsum, Wsum = sum_b w_b over the global batch: the
// loss a user of the reference writes around flow.apply(..., train=True) for
// weighted samples (event weights, sWeights, importance weights; they may be
// zero or negative, their sum must be positive).

// Leaf sums of the fp32 weights, fp64 in row order (leaf_sum_kernel's leaves).
__global__ void leaf_sum_f32_kernel(const float* __restrict__ x, int B, int rows, int n, double* __restrict__ p) {
  const int z = blockIdx.x * blockDim.x + threadIdx.x;
  if (z >= n) return;
  const int b0 = min(B, z * rows), b1 = min(B, b0 + rows);
  double a = 0.0;
  for (int b = b0; b < b1; ++b) a += (double)x[b];
  p[z] = a;
}

// latent_loss_kernel with a weight per row: lp as there (restated, as in
// latent_vjp_kernel: the unweighted kernel keeps its code); the row's loss term
// -w lp / Wsum (fp64: the product is exact, the quotient rounded once); its
// cotangent ce = -w / Wsum (the fp64 quotient, rounded once) where lp is
// finite before nan_to_num and 0 elsewhere (latent_vjp_kernel's `fin` rule),
// which seeds gz = ce . d latent_lp / dz here and the log-det cotangent of
// every coupling's spline reverse.  wsum: the global sum of the weights (one
// double on the device).  The leaf sums as in latent_loss_kernel.
__global__ __launch_bounds__(256) void latent_loss_weighted_kernel(
    const float* __restrict__ z, const float* __restrict__ ld, const float* __restrict__ w,
    const double* __restrict__ wsum, int B, int D, int rot, int latent, float a, float betac, float tnmass,
    float* __restrict__ gz, float* __restrict__ ce, double* __restrict__ row_loss, int leaf_rows, int leaf_n,
    double* __restrict__ leaf) {
  __shared__ double rl[256];
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) {
    float lat = 0.f;
    for (int j = 0; j < D; ++j) {
      const float v = z[(long long)b * D + pmodi(j + rot, D)];
      float t;
      if (latent == ZF_LATENT_NORMAL || latent == ZF_LATENT_TRUNCNORM) {
        const float dv = v - 0.5f;
        t = (logf(6.28318530717958647692f * 0.01f) + (dv * dv) / 0.01f) / -2.0f;
        if (latent == ZF_LATENT_TRUNCNORM) {
          t = t - tnmass;
          if (dv / 0.1f < -5.f || dv / 0.1f > 5.f) t = -INFINITY;
        }
      } else if (latent == ZF_LATENT_BETA) {
        const float am1 = a - 1.0f;
        t = betac + (am1 == 0.f ? 0.f : am1 * logf(v)) + (am1 == 0.f ? 0.f : am1 * log1pf(-v));
        if (v > 1.f || v < 0.f) t = -INFINITY;
      } else {
        t = (v > 1.f || v < 0.f) ? -INFINITY : 0.f;
      }
      lat = lat + t;
    }
    float lp = lat + ld[b];
    const bool fin = (lp == lp) && lp != INFINITY && lp != -INFINITY;
    if (lp != lp) lp = -INFINITY;
    if (lp == INFINITY) lp = 3.40282347e38f;
    if (lp == -INFINITY) lp = -3.40282347e38f;
    const double W = *wsum, wb = (double)w[b];
    const double term = -(wb * (double)lp) / W;
    row_loss[b] = term;
    const float s = fin ? (float)(-wb / W) : 0.f;
    ce[b] = s;
    for (int j = 0; j < D; ++j) {
      const int col = pmodi(j + rot, D);
      const float v = z[(long long)b * D + col];
      float g = 0.f;
      if (fin) {
        if (latent == ZF_LATENT_NORMAL || latent == ZF_LATENT_TRUNCNORM) g = -(v - 0.5f) / 0.01f;
        else if (latent == ZF_LATENT_BETA) g = (a - 1.0f) / v - (a - 1.0f) / (1.0f - v);
      }
      gz[(long long)b * D + col] = s * g;
    }
    rl[threadIdx.x] = term;
  }
  if (leaf_rows <= 0) return;
  __syncthreads();
  const int per = 256 / leaf_rows, z0 = blockIdx.x * 256;
  if ((int)threadIdx.x < per) {
    const int r0 = z0 + threadIdx.x * leaf_rows;
    if (r0 < B) {
      const int r1 = min(B, r0 + leaf_rows);
      double acc = 0.0;
      for (int r = r0; r < r1; ++r) acc += rl[r - z0];
      leaf[r0 / leaf_rows] = acc;
    }
  }
  if (blockIdx.x == gridDim.x - 1)  // the leaves past the last row are empty (0, as leaf_sum_kernel)
    for (int zl = (B + leaf_rows - 1) / leaf_rows + (int)threadIdx.x; zl < leaf_n; zl += 256) leaf[zl] = 0.0;
}

// ShiftBounds batch min / max of every rank (all-gathered [world][2][64]:
// min row, max row) -> the global min / max (a NaN anywhere stays NaN).
__global__ void minmax_ranks_kernel(const float* __restrict__ gath, int world, int D, float* __restrict__ cmin,
                                    float* __restrict__ cmax) {
  const int i = threadIdx.x;
  if (i >= D) return;
  float lo = gath[i], hi = gath[64 + i];
  for (int r = 1; r < world; ++r) {
    const float a = gath[r * 128 + i], b = gath[r * 128 + 64 + i];
    lo = (lo != lo || a != a) ? __builtin_nanf("") : fminf(lo, a);
    hi = (hi != hi || b != b) ? __builtin_nanf("") : fmaxf(hi, b);
  }
  cmin[i] = lo;
  cmax[i] = hi;
}

__device__ __forceinline__ void step_update(float* __restrict__ bc, float b1, float b2);

// bc != NULL: thread 0 also advances the optimiser's step counter (the step
// graph's launch before adam_kernel; step_kernel otherwise).
__global__ void cast_f64_f32_kernel(const double* __restrict__ x, long long n, float* __restrict__ y,
                                    float* __restrict__ bc = nullptr, float b1 = 0.f, float b2 = 0.f) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = (float)x[i];
  if (bc && i == 0) step_update(bc, b1, b2);
}

// ---- optimiser: optax adamw / nadamw ---------------------------------------
// scale_by_adam(b1, b2, eps, nesterov) -> add_decayed_weights(wd) -> scale(-lr)
// (optax/_src/transform.py, alias.py), masked to the parameter entries.
// Step count and bias corrections on the device (so a captured step graph
// replays correctly): bc[0] = step t (as float bits of an int), bc[1] =
// 1 - b1^t, bc[2] = 1 - b1^(t+1), bc[3] = 1 - b2^t.
__device__ __forceinline__ void step_update(float* __restrict__ bc, float b1, float b2) {
  int* cnt = reinterpret_cast<int*>(bc);
  const int t = *cnt + 1;
  *cnt = t;
  bc[1] = (float)(1.0 - pow((double)b1, (double)t));
  bc[2] = (float)(1.0 - pow((double)b1, (double)t + 1.0));
  bc[3] = (float)(1.0 - pow((double)b2, (double)t));
}

__global__ void step_kernel(float* __restrict__ bc, float b1, float b2) { step_update(bc, b1, b2); }

__global__ void adam_kernel(float* __restrict__ prm, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, const unsigned char* __restrict__ mask, long long n, float lr,
                            float b1, float b2, float eps, float wd, int nesterov, const float* __restrict__ bc) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !mask[i]) return;
  const float bc1 = bc[1], bc1n = bc[2], bc2 = bc[3];
  const float gi = g[i];
  const float mi = b1 * m[i] + (1.0f - b1) * gi;
  const float vi = b2 * v[i] + (1.0f - b2) * gi * gi;
  m[i] = mi;
  v[i] = vi;
  // bias corrections: bc1 = 1 - b1^t, bc1n = 1 - b1^(t+1), bc2 = 1 - b2^t
  const float mhat = nesterov ? b1 * (mi / bc1n) + (1.0f - b1) * (gi / bc1) : mi / bc1;
  const float vhat = vi / bc2;
  const float upd = mhat / (sqrtf(vhat) + eps) + wd * prm[i];
  prm[i] = prm[i] - lr * upd;
}

// The latent's constants (latent_loss_kernel, latent_vjp_kernel): the Beta
// log-normaliser and the log mass of the truncated Normal.
struct LatentConsts {
  int lt;
  float a, betac, tnm;
  explicit LatentConsts(const zf_flow_desc& desc)
      : lt(desc.latent),
        a((float)desc.latent_param),
        betac(desc.latent == ZF_LATENT_BETA
                  ? (float)(-(std::lgamma(desc.latent_param) * 2.0 - std::lgamma(2.0 * desc.latent_param)))
                  : 0.f),
        tnm((float)std::log1p(-2.0 * 0.5 * std::erfc(5.0 / std::sqrt(2.0)))) {}
};

// bn_eval_fwd_kernel that also keeps Uhat = (u - mean) rstd, which the
// BatchNorm scale gradient of an eval-mode reverse pass sums against gUbn
// (zf_trainer_forward with train = 0).  Ubn and rstd_out are formed by the
// same separately rounded operations, so they have bn_eval_fwd_kernel's bits.
// Last in this header: the kernels above keep their places in the code object.
__global__ void bn_eval_fwd_uhat_kernel(const float* __restrict__ s, const float* __restrict__ c,
                                        const float* __restrict__ nat_bn, float* __restrict__ Uhat,
                                        float* __restrict__ Ubn, float* __restrict__ rstd_out, int B, int D, int C,
                                        int dt, int dc, int rot) {
  const int DC = dc + C;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)B * DC) return;
  const long long b = i / DC;
  const int k = (int)(i - b * DC);
  const float u = k < dc ? s[b * D + pmodi(dt + k + rot, D)] : c[b * C + (k - dc)];
  const float rstd = 1.0f / sqrtf(nat_bn[DC + k] + kBnEps);
  if (b == 0) rstd_out[k] = rstd;
  const float uh = bn_hat(u, nat_bn[k], rstd);
  Uhat[i] = uh;
  Ubn[i] = bn_out(uh, nat_bn[2 * DC + k], nat_bn[3 * DC + k]);
}

}  // namespace
}  // namespace zf
