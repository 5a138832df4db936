// RQ-spline rows of the trainer and the layered eval path: one thread per
// (row, transformed dim) normalises the raw conditioner outputs and runs the
// spline forward (log_det), inverse or reverse pass; the host launchers.
#pragma once
#include "zf_internal.h"
#include "zf_reduce.h"
#include "zf_spline.h"

namespace zf {
namespace {

constexpr float kEpsT = 1e-5f;       // utils.py:15

// Spline-path arithmetic at a third of the IEEE expansions' instructions (the
// per-thread spline kernels are issue-latency bound: one wave per (row block),
// thousands of dependent VALU): a hardware reciprocal / square root with one
// Newton or residual step, and quotients by a loop-invariant divisor as one
// residual correction of x * rcp(d) — the correctly rounded result for these
// normal operands, as zf_flow_dev.h's div_cr in the inference kernels.
__device__ __forceinline__ float t_rcp(float x) {
  const float r = __builtin_amdgcn_rcpf(x);
  return __builtin_fmaf(__builtin_fmaf(-x, r, 1.0f), r, r);
}
__device__ __forceinline__ float t_div(float x, float d, float r) {
  const float q = x * r;
  return __builtin_fmaf(__builtin_fmaf(-q, d, x), r, q);
}
// sqrt(x^2 + 4) (>= 2: never denormal), residual-corrected hardware root
__device__ __forceinline__ float t_sq4(float x) {
  const float a = x * x + 4.0f;
  const float sq = __builtin_amdgcn_sqrtf(a);
  return __builtin_fmaf(__builtin_fmaf(-sq, sq, a), 0.5f * __builtin_amdgcn_rcpf(sq), sq);
}
__device__ __forceinline__ float sp_f(float x) { return 0.5f * (x + t_sq4(x)); }
__device__ __forceinline__ float sp_grad(float x) {
  const float sq = t_sq4(x);
  return 0.5f * (1.0f + t_div(x, sq, t_rcp(sq)));
}

constexpr int kMaxK = 64;

// One (row, transformed dim): normalize_spline_params (utils.py:37-62) of the
// raw conditioner outputs p[0..3K-1), bin, RQ spline forward (utils.py:65-141).
// With grads: reverse pass for gy (dL/dy) and gl (dL/dlog_det): dL/dx and dL/dp.
// No per-thread arrays (they would live in scratch): the normalised widths and
// heights are recomputed from p where needed, in the same float order.
// gp may alias p (in-place reverse): every p[j] is read before gp[j] is written.
// KT > 0: the knot count at compile time (8, 16, 32: every loop unrolled, so
// the per-knot squareplus / divisions of different knots overlap instead of
// running as one long dependent chain).  The same operations in the same
// order as KT = 0 (the runtime-K form for other counts), but not always the
// same bits: fp contraction may pair a multiply with a different add once
// the loops are unrolled.  Every rank runs the same form, so the
// data-parallel bit-identity holds.
template <bool GRAD, int KT = 0>
__device__ __forceinline__ void spline_one(const float* p, int Kr, float x, float& y, float& ld, float gy, float gl,
                                           float* gx, float* gp) {
  constexpr int U = KT > 0 ? KT + 1 : 1;  // unroll counts (1: as written)
  const int K = KT > 0 ? KT : Kr;
  const double c64 = 1e-5 / (1.0 - (double)K * 1e-5);  // utils.py:32-34, Python floats
  const float cc = (float)c64, norm = (float)(1.0 + c64 * (double)K);
  float Sa = 0.f, Sb = 0.f;
#pragma unroll U
  for (int j = 0; j < K; ++j) {
    Sa = Sa + sp_f(p[j]);
    Sb = Sb + sp_f(p[K + j]);
  }
  // bin: count semantics of _index (utils.py:244-250); the knots t_j are
  // non-decreasing, so the last knot <= x is knot cnt - 1 and its prefix sums
  // are the bin's left edge (xk, yk)
  float xk = 0.f, yk = 0.f;
  int cnt = 0;
  const float rSa = t_rcp(Sa), rSb = t_rcp(Sb), rnorm = t_rcp(norm);
  {
    float tx = 0.f, ty = 0.f;
#pragma unroll U
    for (int j = 0; j <= K; ++j) {
      if (tx <= x) {
        ++cnt;
        xk = tx;
        yk = ty;
      }
      if (j < K) {
        tx = tx + t_div(t_div(sp_f(p[j]), Sa, rSa) + cc, norm, rnorm);
        ty = ty + t_div(t_div(sp_f(p[K + j]), Sb, rSb) + cc, norm, rnorm);
      }
    }
  }
  int idx = cnt - 1;
  idx = idx < 0 ? 0 : (idx > K ? K : idx);
  if (cnt == 0) xk = yk = 0.f;
  const bool oob = (x < 0.f) || (x >= 1.f);
  if (idx == K || oob) {
    // idx == K: the reference's fill-mode gather gives NaN (utils.py:224-230);
    // oob rows are the identity with log_det 0 (:130, :138).
    y = oob ? x : __builtin_nanf("");
    ld = oob ? 0.f : __builtin_nanf("");
    if (GRAD) {
      *gx = oob ? gy : __builtin_nanf("");
#pragma unroll U
      for (int j = 0; j < 3 * K - 1; ++j) gp[j] = 0.f;
    }
    return;
  }
  const float wk = t_div(t_div(sp_f(p[idx]), Sa, rSa) + cc, norm, rnorm);
  const float hk = t_div(t_div(sp_f(p[K + idx]), Sb, rSb) + cc, norm, rnorm);
  const float dk = (idx == 0) ? 1.f : sp_f(p[2 * K + idx - 1]);
  const float dk1 = (idx + 1 == K) ? 1.f : sp_f(p[2 * K + idx]);
  const float rwk = t_rcp(wk);
  const float sk = t_div(hk, wk, rwk);
  const float zr = t_div(x - xk, wk, rwk);
  const float z = fminf(fmaxf(zr, kEpsT), 0.99999f);
  const float az = 1.0f - z;
  const float num = hk * z * (sk * z + dk * az);
  const float den = sk + (dk1 + dk - 2.0f * sk) * z * az;
  const float dE = den + kEpsT, rdE = t_rcp(dE);
  y = yk + t_div(num, dE, rdE);
  const float q = z * (dk1 * z + 2.0f * sk * az) + dk * (az * az);
  ld = 2.0f * logf(sk + kEpsT) + logf(q + kEpsT) - 2.0f * logf(den + kEpsT);
  if (!GRAD) return;
  // ---- reverse pass ----
  float g_yk = gy;
  const float g_num = t_div(gy, dE, rdE);
  const float dE2 = dE * dE, skE = sk + kEpsT, qE = q + kEpsT;
  float g_den = t_div(-gy * num, dE2, t_rcp(dE2)) - t_div(2.0f * gl, dE, rdE);
  float g_sk = t_div(2.0f * gl, skE, t_rcp(skE));
  const float g_q = t_div(gl, qE, t_rcp(qE));
  float g_hk = g_num * (sk * z * z + dk * z * az);
  g_sk += g_num * hk * z * z;
  float g_dk = g_num * hk * z * az;
  float g_z = g_num * hk * (2.0f * sk * z + dk * (az - z));
  g_sk += g_den * (1.0f - 2.0f * z * az);
  float g_dk1 = g_den * z * az;
  g_dk += g_den * z * az;
  g_z += g_den * (dk1 + dk - 2.0f * sk) * (az - z);
  g_dk1 += g_q * z * z;
  g_sk += g_q * 2.0f * z * az;
  g_dk += g_q * az * az;
  g_z += g_q * (2.0f * dk1 * z + 2.0f * sk * (az - z) - 2.0f * dk * az);
  const float g_zr = (zr > kEpsT && zr < 0.99999f) ? g_z : 0.f;  // jnp.clip passes inside only
  *gx = t_div(g_zr, wk, rwk);
  const float g_xk = t_div(-g_zr, wk, rwk);
  float g_wk = t_div(-g_zr * zr, wk, rwk);
  g_hk += t_div(g_sk, wk, rwk);
  const float wk2 = wk * wk;
  g_wk += t_div(-g_sk * hk, wk2, t_rcp(wk2));
  // gradient w.r.t. widths / heights: xk = sum_{j<idx} w_j (likewise yk), plus
  // the bin's own w_idx, h_idx; then through w_j = (sa_j / Sa + c) / norm
  auto gw = [&](int j) { return j < idx ? g_xk : (j == idx ? g_wk : 0.f); };
  auto gh = [&](int j) { return j < idx ? g_yk : (j == idx ? g_hk : 0.f); };
  float tw = 0.f, th = 0.f;
#pragma unroll U
  for (int j = 0; j < K; ++j) {
    tw += gw(j) * sp_f(p[j]);
    th += gh(j) * sp_f(p[K + j]);
  }
  const float gd0 = idx >= 1 ? g_dk * sp_grad(p[2 * K + idx - 1]) : 0.f;
  const float gd1 = idx + 1 < K ? g_dk1 * sp_grad(p[2 * K + idx]) : 0.f;
  const float Sa2 = Sa * Sa, Sb2 = Sb * Sb;
  const float twq = t_div(tw, Sa2, t_rcp(Sa2)), thq = t_div(th, Sb2, t_rcp(Sb2));
#pragma unroll U
  for (int j = 0; j < K; ++j) {
    const float gsa = t_div(t_div(gw(j), Sa, rSa) - twq, norm, rnorm);
    const float gsb = t_div(t_div(gh(j), Sb, rSb) - thq, norm, rnorm);
    gp[j] = gsa * sp_grad(p[j]);
    gp[K + j] = gsb * sp_grad(p[K + j]);
  }
#pragma unroll U
  for (int j = 0; j < K - 1; ++j) gp[2 * K + j] = 0.f;
  if (idx >= 1) gp[2 * K + idx - 1] = 0.f + gd0;
  if (idx + 1 < K) gp[2 * K + idx] = 0.f + gd1;
}

// Thread per (row, transformed dim): one-wave blocks of rpb = 64 / dt rows.
// The block's conditioner outputs P[b0 .. b0+rpb)[dt][S] are contiguous: they
// are staged through LDS with coalesced loads (thread-major [64][S], S odd for
// even K so the per-thread rows spread over the banks).  Logical dim d < dt is
// column pmod(d + rot, D); thread d also carries the conditioning columns
// dt + d, dt + d + dt, ... through unchanged.
constexpr int kSplThreads = 64;

// Launch LAUNCH(KT) with the compile-time knot count where instantiated.
#define ZF_KNOT_DISPATCH(K, LAUNCH) \
  do {                              \
    if ((K) == 8) LAUNCH(8);        \
    else if ((K) == 16) LAUNCH(16); \
    else if ((K) == 32) LAUNCH(32); \
    else LAUNCH(0);                 \
  } while (0)

// Global <-> LDS copies of n floats, kStageInflight loads in flight per lane
// (the per-thread spline kernels run one wave per block: every serial HBM
// round trip here is exposed — 48 in flight stage K = 16's 47 floats per
// lane in one round instead of six).
constexpr int kStageInflight = 48;
__device__ __forceinline__ void stage_rows(float* sp, const float* __restrict__ src, long long n) {
  for (long long e0 = threadIdx.x; e0 < n; e0 += kStageInflight * kSplThreads) {
    float v[kStageInflight];
#pragma unroll
    for (int u = 0; u < kStageInflight; ++u) {
      const long long e = e0 + u * kSplThreads;
      v[u] = e < n ? src[e] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kStageInflight; ++u) {
      const long long e = e0 + u * kSplThreads;
      if (e < n) sp[e] = v[u];
    }
  }
}

__device__ __forceinline__ void unstage_rows(float* __restrict__ dst, const float* sp, long long n) {
  for (long long e0 = threadIdx.x; e0 < n; e0 += 8 * kSplThreads) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const long long e = e0 + u * kSplThreads;
      if (e < n) dst[e] = sp[e];
    }
  }
}

// Forward: log-det summed per row in dim order through LDS.
template <int KT>
__global__ __launch_bounds__(kSplThreads) void spline_fwd_kernel(const float* __restrict__ s_in,
                                                                 float* __restrict__ s_out,
                                                                 const float* __restrict__ P, float* __restrict__ ld,
                                                                 int B, int D, int dt, int K, int rot) {
  extern __shared__ float sp[];
  __shared__ float lds[kSplThreads];
  const int S = 3 * K - 1, rpb = kSplThreads / dt;
  const int lr = threadIdx.x / dt, d = threadIdx.x - lr * dt;
  const long long b0 = (long long)blockIdx.x * rpb, b = b0 + lr;
  const int nrows = (int)(B - b0 < rpb ? B - b0 : rpb);
  const bool ok = lr < nrows;
  const int col = pmodi(d + rot, D);
  const float xv = ok ? s_in[b * D + col] : 0.f;  // in flight with the staging loads
  stage_rows(sp, P + b0 * dt * S, (long long)nrows * dt * S);
  __syncthreads();
  if (ok) {
    for (int j = dt + d; j < D; j += dt) {
      const int cj = pmodi(j + rot, D);
      s_out[b * D + cj] = s_in[b * D + cj];
    }
    float y, ldv;
    spline_one<false, KT>(sp + threadIdx.x * S, K, xv, y, ldv, 0.f, 0.f, nullptr, nullptr);
    s_out[b * D + col] = y;
    lds[threadIdx.x] = ldv;
  }
  __syncthreads();
  if (ok && d == 0) {
    float l = 0.f;
    for (int k = 0; k < dt; ++k) l = l + lds[threadIdx.x + k];
    ld[b] = ld[b] + l;
  }
}

// Inverse (the layered eval path's Chain.inverse; utils.py:144-202): the same
// per-(row, dim) layout and staging; knots normalized as spline_one forms
// them, bin search and quadratic root as the fused kernels (zf_spline.h).
struct RawKnots {
  const float* p;
  int K;
  float Sa, Sb, rSa, rSb, cc, norm, rnorm;
  __device__ float w(int j) const { return t_div(t_div(sp_f(p[j]), Sa, rSa) + cc, norm, rnorm); }
  __device__ float h(int j) const { return t_div(t_div(sp_f(p[K + j]), Sb, rSb) + cc, norm, rnorm); }
  __device__ float d(int j) const { return sp_f(p[2 * K + j]); }
};

__device__ __forceinline__ float spline_inv_one(const float* p, int K, float y) {
  RawKnots q;
  q.p = p;
  q.K = K;
  const double c64 = 1e-5 / (1.0 - (double)K * 1e-5);  // utils.py:32-34, Python floats
  q.cc = (float)c64;
  q.norm = (float)(1.0 + c64 * (double)K);
  float Sa = 0.f, Sb = 0.f;
  for (int j = 0; j < K; ++j) {
    Sa = Sa + sp_f(p[j]);
    Sb = Sb + sp_f(p[K + j]);
  }
  q.Sa = Sa;
  q.Sb = Sb;
  q.rSa = t_rcp(Sa);
  q.rSb = t_rcp(Sb);
  q.rnorm = t_rcp(q.norm);
  const RqsBin b = rqs_bin<false>(y, K, q);
  return rqs_inverse_eval(y, b);
}

__global__ __launch_bounds__(kSplThreads) void spline_inv_kernel(const float* __restrict__ s_in,
                                                                 float* __restrict__ s_out,
                                                                 const float* __restrict__ P, int B, int D, int dt,
                                                                 int K, int rot) {
  extern __shared__ float sp[];
  const int S = 3 * K - 1, rpb = kSplThreads / dt;
  const int lr = threadIdx.x / dt, d = threadIdx.x - lr * dt;
  const long long b0 = (long long)blockIdx.x * rpb, b = b0 + lr;
  const int nrows = (int)(B - b0 < rpb ? B - b0 : rpb);
  const bool ok = lr < nrows;
  const int col = pmodi(d + rot, D);
  const float yv = ok ? s_in[b * D + col] : 0.f;
  stage_rows(sp, P + b0 * dt * S, (long long)nrows * dt * S);
  __syncthreads();
  if (!ok) return;
  for (int j = dt + d; j < D; j += dt) {
    const int cj = pmodi(j + rot, D);
    s_out[b * D + cj] = s_in[b * D + cj];
  }
  s_out[b * D + col] = spline_inv_one(sp + threadIdx.x * S, K, yv);
}

// Reverse: g_in = dL/d(state_in) from g_out = dL/d(state_out) and gl per row;
// conditioning columns pass g_out through (their MLP share is added later).
// dL/dP is formed in place in the staged rows and written back coalesced.
// ROWGL (the eval-mode vector-Jacobian product, where every row has its own
// cotangent): gl of row b is glr[b]; otherwise the constant gl, as before.
template <int KT, bool ROWGL = false>
__global__ __launch_bounds__(kSplThreads) void spline_bwd_kernel(const float* __restrict__ s_in,
                                                                 const float* __restrict__ P,
                                                                 const float* __restrict__ g_out, float gl,
                                                                 float* __restrict__ g_in, float* __restrict__ gP,
                                                                 int B, int D, int dt, int K, int rot,
                                                                 const float* __restrict__ glr = nullptr) {
  extern __shared__ float sp[];
  const int S = 3 * K - 1, rpb = kSplThreads / dt;
  const int lr = threadIdx.x / dt, d = threadIdx.x - lr * dt;
  const long long b0 = (long long)blockIdx.x * rpb, b = b0 + lr;
  const int nrows = (int)(B - b0 < rpb ? B - b0 : rpb);
  const long long n = (long long)nrows * dt * S;
  const bool ok = lr < nrows;
  const int col = pmodi(d + rot, D);
  const float xv = ok ? s_in[b * D + col] : 0.f, gv = ok ? g_out[b * D + col] : 0.f;  // in flight with the staging
  float glv = gl;
  if constexpr (ROWGL) glv = ok ? glr[b] : 0.f;
  stage_rows(sp, P + b0 * dt * S, n);
  __syncthreads();
  if (ok) {
    for (int j = dt + d; j < D; j += dt) {
      const int cj = pmodi(j + rot, D);
      g_in[b * D + cj] = g_out[b * D + cj];
    }
    float y, ldv, gx;
    float* row = sp + threadIdx.x * S;
    spline_one<true, KT>(row, K, xv, y, ldv, gv, glv, &gx, row);
    g_in[b * D + col] = gx;
  }
  __syncthreads();
  unstage_rows(gP + b0 * dt * S, sp, n);
}

// The forward spline of B rows: one-wave blocks of 64 / dt rows, each row's dt * (3K - 1)
// parameters staged in LDS.
int spline_fwd_launch(const float* s_in, float* s_out, const float* P, float* ld, int B, int D, int dt, int K,
                      int rot, hipStream_t st) {
  const int rpb = kSplThreads / dt;
  const size_t lds = (size_t)kSplThreads * (3 * K - 1) * sizeof(float);
#define ZF_SPL(KTV)                                                                                          \
  hipLaunchKernelGGL((spline_fwd_kernel<KTV>), dim3(blocks_for(B, rpb)), dim3(kSplThreads), lds, st, s_in, \
                     s_out, P, ld, B, D, dt, K, rot)
  ZF_KNOT_DISPATCH(K, ZF_SPL);
#undef ZF_SPL
  ZF_CHECK_LAUNCH("spline_fwd_kernel");
  return ZF_OK;
}

// Its reverse: g_out -> g_in (transformed columns) and gP.  d loss / d log_det is gl for
// every row, or (ROWGL) row b's is glr[b].
template <bool ROWGL>
int spline_bwd_launch(const float* s_in, const float* P, const float* g_out, float gl, float* g_in, float* gP, int B,
                      int D, int dt, int K, int rot, const float* glr, hipStream_t st) {
  const int rpb = kSplThreads / dt;
  const size_t lds = (size_t)kSplThreads * (3 * K - 1) * sizeof(float);
#define ZF_SPL(KTV)                                                                                                 \
  hipLaunchKernelGGL((spline_bwd_kernel<KTV, ROWGL>), dim3(blocks_for(B, rpb)), dim3(kSplThreads), lds, st, s_in, \
                     P, g_out, gl, g_in, gP, B, D, dt, K, rot, glr)
  ZF_KNOT_DISPATCH(K, ZF_SPL);
#undef ZF_SPL
  ZF_CHECK_LAUNCH(ROWGL ? "spline_bwd_kernel<rowgl>" : "spline_bwd_kernel");
  return ZF_OK;
}

// spline_rows (zf_internal.h): forward with log_det += into ld, or inverse.
int spline_rows_launch(bool inverse, const float* s_in, float* s_out, const float* P, float* ld, int B, int D, int dt,
                       int K, int rot, hipStream_t st) {
  if (B <= 0) return ZF_OK;
  // the layered eval path takes up to 200 knots (the block's rows of 3K - 1
  // parameters staged in LDS: 64 x 599 floats); training stays at kMaxK
  if (dt < 1 || dt > kSplThreads || K < 1 || K > 200) return enotsup("spline rows: transformed dims or knots out of range");
  if (!inverse) return spline_fwd_launch(s_in, s_out, P, ld, B, D, dt, K, rot, st);
  const int S = 3 * K - 1, rpb = kSplThreads / dt;
  const size_t lds = (size_t)kSplThreads * S * sizeof(float);
  hipLaunchKernelGGL(spline_inv_kernel, dim3(blocks_for(B, rpb)), dim3(kSplThreads), lds, st, s_in, s_out, P, B,
                     D, dt, K, rot);
  ZF_CHECK_LAUNCH("spline_inv_kernel");
  return ZF_OK;
}

}  // namespace
}  // namespace zf
