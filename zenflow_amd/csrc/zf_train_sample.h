// Gradients through sampling (zf_trainer_sample_forward / _backward): the RQ
// spline inverse as a differentiable op, ShiftBounds.inverse and its reverse,
// and the small row kernels of the pass.  One translation unit of its own
// (zf_sample_grad.hip): the trainer's code object keeps its bytes.
//
// The inverse pass walks the chain from the latent to the data.  For one
// coupling it maps the op's forward OUTPUT state (y_t, conditioning columns)
// to its forward INPUT state (x_t, the same conditioning columns):
//   x_t = rational_quadratic_spline_inverse(y_t; P)        utils.py:144-202
// with P the raw conditioner outputs of the conditioning columns, and the
// row's log_q gains the op's forward log-det at that x_t (utils.py:121-139).
#pragma once
#include "zf_train_spline.h"

namespace zf {
namespace {

__device__ __forceinline__ bool finitef(float v) { return (v == v) && v != INFINITY && v != -INFINITY; }

// ---- forward: x_t and the forward log-det at x_t -----------------------------
// One (row, transformed dim): x as spline_inv_one forms it (the same bits), and
// the forward spline's log-det (utils.py:121-139) at that x.  The forward's
// z = (x - xk) / wk is the inverse's own root, known before x = z wk + xk is
// rounded: the log-det is formed from it directly (clamped as the forward
// clamps it) on the bin the inverse found, without a second sweep over the
// knots and without the cancellation in x - xk.
__device__ __forceinline__ void spline_inv_ld_one(const float* p, int K, float y, float& x, float& ld) {
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
  x = rqs_inverse_eval(y, b);
  // the root of rqs_inverse_eval, again (utils.py:193-197)
  const float dy = y - b.yk;
  const float t = b.dkp1 + b.dk - 2.0f * b.sk;
  const float a = b.h * (b.sk - b.dk) + dy * t;
  const float bb = b.h * b.dk - dy * t;
  const float c = -b.sk * dy;
  const float zr = 2.0f * c / (-bb - __builtin_sqrtf(bb * bb - 4.0f * a * c));
  const float z = (zr != zr) ? zr : fminf(fmaxf(zr, kEps), kOneMinusEps);
  const float az = 1.0f - z;
  const float den = b.sk + t * z * az;
  const float num2 = z * (b.dkp1 * z + 2.0f * b.sk * az) + b.dk * (az * az);
  const float l = 2.0f * logf(b.sk + kEps) + logf(num2 + kEps) - 2.0f * logf(den + kEps);
  ld = b.oob ? 0.0f : l;
}

// spline_inv_kernel's layout and staging.  ld[b] gains the row's log-det in dim
// order through LDS, as spline_fwd_kernel adds it.  A lane whose x_t is not
// finite (the idx == K sliver on the yk knots: the reference's fill-mode NaN)
// marks its row in dead[] and stores 0.5 in the state instead, so that the
// conditioners of the ops still to come, whose activations the reverse pass
// multiplies by that row's zero cotangents, stay finite; the row's x is
// written as NaN at the end of the pass (sb_eval_inv_kernel).
template <int KT>
__global__ __launch_bounds__(kSplThreads) void spline_inv_ld_kernel(const float* __restrict__ s_in,
                                                                    float* __restrict__ s_out,
                                                                    const float* __restrict__ P,
                                                                    float* __restrict__ ld, float* __restrict__ dead,
                                                                    int B, int D, int dt, int K, int rot) {
  extern __shared__ float sp[];
  __shared__ float lds[kSplThreads];
  const int S = 3 * K - 1, rpb = kSplThreads / dt;
  const int lr = threadIdx.x / dt, d = threadIdx.x - lr * dt;
  const long long b0 = (long long)blockIdx.x * rpb, b = b0 + lr;
  const int nrows = (int)(B - b0 < rpb ? B - b0 : rpb);
  const bool ok = lr < nrows;
  const int col = pmodi(d + rot, D);
  const float yv = ok ? s_in[b * D + col] : 0.f;  // in flight with the staging loads
  stage_rows(sp, P + b0 * dt * S, (long long)nrows * dt * S);
  __syncthreads();
  if (ok) {
    for (int j = dt + d; j < D; j += dt) {
      const int cj = pmodi(j + rot, D);
      s_out[b * D + cj] = s_in[b * D + cj];
    }
    const float* row = sp + threadIdx.x * S;
    float xv, ldv;
    spline_inv_ld_one(row, KT > 0 ? KT : K, yv, xv, ldv);
    if (!finitef(xv)) {
      dead[b] = 1.0f;  // every lane of the row that gets here stores the same value
      xv = 0.5f;
      ldv = __builtin_nanf("");
    }
    s_out[b * D + col] = xv;
    lds[threadIdx.x] = ldv;
  }
  __syncthreads();
  if (ok && d == 0) {
    float l = 0.f;
    for (int k = 0; k < dt; ++k) l = l + lds[threadIdx.x + k];
    ld[b] = ld[b] + l;
  }
}

// ---- reverse of one (row, transformed dim) ------------------------------------
// Inputs: the raw parameters p[0..3K-1), y (the inverse's input), x (its
// output), gxo = d L / d x and gl = d L / d log_q of the row.  Outputs: *gy =
// d L / d y and gp = d L / d p (gp may alias p: every p[j] is read before
// gp[j] is written).
//
// Two paths meet in the six bin-level cotangents (xk, yk, wk, hk, dk, dk1):
//   log_q  the forward spline's log-det at x, reversed as spline_one<true>
//          reverses it with gy = 0: bin on the xk knots, z clamped, the
//          epsilons of utils.py:121-139.  Its d / d x joins gxo.
//   x      the derivative of the inverse's own formula (utils.py:193-201):
//          bin on the yk knots, sk = hk / wk, dy = y - yk,
//            t = dk1 + dk - 2 sk,  a = hk (sk - dk) + dy t,  b = hk dk - dy t,
//            c = -sk dy,  z = 2c / (-b - sqrt(b^2 - 4ac)),  x = z wk + xk
//          reversed term by term: no clamp, no epsilons.  (1 / s'(x) of the
//          forward spline is not this derivative: the forward carries
//          den + 1e-5 and the clamp.)
// The two bins are the same bin except where rounding puts x across a knot;
// each path scatters with its own index, and the softmax / squareplus tail of
// spline_one runs once over the sums.  No per-thread arrays.
template <int KT>
__device__ __forceinline__ void spline_inv_grad_one(const float* p, int Kr, float y, float x, float gxo, float gl,
                                                    float* gy, float* gp) {
  constexpr int U = KT > 0 ? KT + 1 : 1;
  const int K = KT > 0 ? KT : Kr;
  const double c64 = 1e-5 / (1.0 - (double)K * 1e-5);  // utils.py:32-34, Python floats
  const float cc = (float)c64, norm = (float)(1.0 + c64 * (double)K);
  float Sa = 0.f, Sb = 0.f;
#pragma unroll U
  for (int j = 0; j < K; ++j) {
    Sa = Sa + sp_f(p[j]);
    Sb = Sb + sp_f(p[K + j]);
  }
  const float rSa = t_rcp(Sa), rSb = t_rcp(Sb), rnorm = t_rcp(norm);
  // one sweep over the knots (the sums spline_one and spline_inv_one form):
  // the inverse's bin by yk <= y, the forward's by xk <= x
  float yki = 0.f, xkf = 0.f;
  int cnti = 0, cntf = 0;
  {
    float tx = 0.f, ty = 0.f;
#pragma unroll U
    for (int j = 0; j <= K; ++j) {
      if (ty <= y) {
        ++cnti;
        yki = ty;
      }
      if (tx <= x) {
        ++cntf;
        xkf = tx;
      }
      if (j < K) {
        tx = tx + t_div(t_div(sp_f(p[j]), Sa, rSa) + cc, norm, rnorm);
        ty = ty + t_div(t_div(sp_f(p[K + j]), Sb, rSb) + cc, norm, rnorm);
      }
    }
  }
  int idi = cnti - 1, idf = cntf - 1;
  idi = idi < 0 ? 0 : (idi > K ? K : idi);
  idf = idf < 0 ? 0 : (idf > K ? K : idf);
  const bool oni = !((y < 0.f) || (y >= 1.f)) && idi < K;  // out of bounds: the identity
  const bool onf = !((x < 0.f) || (x >= 1.f)) && idf < K;  // out of bounds: log-det 0
  // ---- log_q: the forward log-det at x, d / d (x, bin) ----
  float gx_ld = 0.f, f_xk = 0.f, f_wk = 0.f, f_hk = 0.f, f_dk = 0.f, f_dk1 = 0.f;
  if (onf) {
    const float wk = t_div(t_div(sp_f(p[idf]), Sa, rSa) + cc, norm, rnorm);
    const float hk = t_div(t_div(sp_f(p[K + idf]), Sb, rSb) + cc, norm, rnorm);
    const float dk = (idf == 0) ? 1.f : sp_f(p[2 * K + idf - 1]);
    const float dk1 = (idf + 1 == K) ? 1.f : sp_f(p[2 * K + idf]);
    const float rwk = t_rcp(wk);
    const float sk = t_div(hk, wk, rwk);
    const float zr = t_div(x - xkf, wk, rwk);
    const float z = fminf(fmaxf(zr, kEpsT), 0.99999f);
    const float az = 1.0f - z;
    const float den = sk + (dk1 + dk - 2.0f * sk) * z * az;
    const float dE = den + kEpsT;
    const float q = z * (dk1 * z + 2.0f * sk * az) + dk * (az * az);
    const float skE = sk + kEpsT, qE = q + kEpsT;
    const float g_den = -t_div(2.0f * gl, dE, t_rcp(dE));
    float g_sk = t_div(2.0f * gl, skE, t_rcp(skE));
    const float g_q = t_div(gl, qE, t_rcp(qE));
    g_sk += g_den * (1.0f - 2.0f * z * az);
    f_dk1 = g_den * z * az;
    f_dk = g_den * z * az;
    float g_z = g_den * (dk1 + dk - 2.0f * sk) * (az - z);
    f_dk1 += g_q * z * z;
    g_sk += g_q * 2.0f * z * az;
    f_dk += g_q * az * az;
    g_z += g_q * (2.0f * dk1 * z + 2.0f * sk * (az - z) - 2.0f * dk * az);
    const float g_zr = (zr > kEpsT && zr < 0.99999f) ? g_z : 0.f;  // jnp.clip passes inside only
    gx_ld = t_div(g_zr, wk, rwk);
    f_xk = -gx_ld;
    f_wk = t_div(-g_zr * zr, wk, rwk);
    f_hk = t_div(g_sk, wk, rwk);
    const float wk2 = wk * wk;
    f_wk += t_div(-g_sk * hk, wk2, t_rcp(wk2));
  }
  // ---- x: the root formula, d / d (y, bin) ----
  const float gxt = gxo + gx_ld;
  float i_xk = 0.f, i_yk = 0.f, i_wk = 0.f, i_hk = 0.f, i_dk = 0.f, i_dk1 = 0.f;
  *gy = oni ? 0.f : ((y < 0.f) || (y >= 1.f) ? gxt : 0.f);
  if (oni) {
    const float wk = t_div(t_div(sp_f(p[idi]), Sa, rSa) + cc, norm, rnorm);
    const float hk = t_div(t_div(sp_f(p[K + idi]), Sb, rSb) + cc, norm, rnorm);
    const float dk = (idi == 0) ? 1.f : sp_f(p[2 * K + idi - 1]);
    const float dk1 = (idi + 1 == K) ? 1.f : sp_f(p[2 * K + idi]);
    const float rwk = t_rcp(wk);
    const float sk = hk / wk;  // as rqs_bin forms it
    const float dy = y - yki;
    const float t = dk1 + dk - 2.0f * sk;
    const float a = hk * (sk - dk) + dy * t;
    const float bq = hk * dk - dy * t;
    const float c = -sk * dy;
    const float r = __builtin_sqrtf(bq * bq - 4.0f * a * c);
    const float den = -bq - r, rden = t_rcp(den);
    const float z = t_div(2.0f * c, den, rden);
    // x = z wk + xk
    const float g_z = gxt * wk;
    i_wk = gxt * z;
    i_xk = gxt;
    // z = 2c / den
    float g_c = t_div(2.0f * g_z, den, rden);
    const float g_dn = -t_div(g_z * z, den, rden);
    // den = -b - r, r = sqrt(b^2 - 4ac)
    const float g_disc = -g_dn * 0.5f * t_rcp(r);
    const float g_b = -g_dn + 2.0f * bq * g_disc;
    const float g_a = -4.0f * c * g_disc;
    g_c += -4.0f * a * g_disc;
    // c = -sk dy ; b = hk dk - dy t ; a = hk (sk - dk) + dy t
    float g_sk = -dy * g_c + hk * g_a;
    float g_dy = -sk * g_c - t * g_b + t * g_a;
    const float g_t = dy * (g_a - g_b);
    i_hk = dk * g_b + (sk - dk) * g_a;
    i_dk = hk * (g_b - g_a) + g_t;
    i_dk1 = g_t;
    g_sk += -2.0f * g_t;
    // dy = y - yk ; sk = hk / wk
    *gy = g_dy;
    i_yk = -g_dy;
    i_hk += t_div(g_sk, wk, rwk);
    const float wk2 = wk * wk;
    i_wk += t_div(-g_sk * hk, wk2, t_rcp(wk2));
  }
  // ---- widths / heights: xk = sum_{j<idx} w_j (likewise yk) plus the bin's own,
  // then through w_j = (sa_j / Sa + c) / norm; slopes through squareplus ----
  auto gw = [&](int j) {
    return (j < idi ? i_xk : (j == idi ? i_wk : 0.f)) + (j < idf ? f_xk : (j == idf ? f_wk : 0.f));
  };
  auto gh = [&](int j) { return (j < idi ? i_yk : (j == idi ? i_hk : 0.f)) + (j == idf ? f_hk : 0.f); };
  float tw = 0.f, th = 0.f;
#pragma unroll U
  for (int j = 0; j < K; ++j) {
    tw += gw(j) * sp_f(p[j]);
    th += gh(j) * sp_f(p[K + j]);
  }
  const float gi0 = (oni && idi >= 1) ? i_dk * sp_grad(p[2 * K + idi - 1]) : 0.f;
  const float gi1 = (oni && idi + 1 < K) ? i_dk1 * sp_grad(p[2 * K + idi]) : 0.f;
  const float gf0 = (onf && idf >= 1) ? f_dk * sp_grad(p[2 * K + idf - 1]) : 0.f;
  const float gf1 = (onf && idf + 1 < K) ? f_dk1 * sp_grad(p[2 * K + idf]) : 0.f;
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
  if (oni && idi >= 1) gp[2 * K + idi - 1] += gi0;
  if (oni && idi + 1 < K) gp[2 * K + idi] += gi1;
  if (onf && idf >= 1) gp[2 * K + idf - 1] += gf0;
  if (onf && idf + 1 < K) gp[2 * K + idf] += gf1;
}

// Reverse of one coupling of the inverse pass.  s_y: the op's input state on
// the inverse pass (y_t), s_x: its output state (x_t), g_out: d L / d s_x,
// glr: d L / d log_q per row (zero on masked rows), mask: 0 on rows that
// contribute nothing.  g_in = d L / d s_y for the transformed columns, the
// conditioning columns pass g_out through (their conditioner share is added
// later); gP is formed in place in the staged rows and written back
// coalesced, as spline_bwd_kernel does.  A masked row writes exact zeros to
// every column of g_in and to its gP rows, whatever its intermediates hold.
template <int KT>
__global__ __launch_bounds__(kSplThreads) void spline_inv_bwd_kernel(
    const float* __restrict__ s_y, const float* __restrict__ s_x, const float* __restrict__ P,
    const float* __restrict__ g_out, const float* __restrict__ glr, const float* __restrict__ mask,
    float* __restrict__ g_in, float* __restrict__ gP, int B, int D, int dt, int K, int rot) {
  extern __shared__ float sp[];
  const int S = 3 * K - 1, rpb = kSplThreads / dt;
  const int lr = threadIdx.x / dt, d = threadIdx.x - lr * dt;
  const long long b0 = (long long)blockIdx.x * rpb, b = b0 + lr;
  const int nrows = (int)(B - b0 < rpb ? B - b0 : rpb);
  const long long n = (long long)nrows * dt * S;
  const bool ok = lr < nrows;
  const int col = pmodi(d + rot, D);
  // in flight with the staging loads
  const float yv = ok ? s_y[b * D + col] : 0.f, xv = ok ? s_x[b * D + col] : 0.f;
  const float gv = ok ? g_out[b * D + col] : 0.f, glv = ok ? glr[b] : 0.f, mv = ok ? mask[b] : 0.f;
  stage_rows(sp, P + b0 * dt * S, n);
  __syncthreads();
  if (ok) {
    const bool live = mv != 0.f;
    for (int j = dt + d; j < D; j += dt) {
      const int cj = pmodi(j + rot, D);
      g_in[b * D + cj] = live ? g_out[b * D + cj] : 0.f;
    }
    float* row = sp + threadIdx.x * S;
    float gy = 0.f;
    if (live) {
      spline_inv_grad_one<KT>(row, K, yv, xv, gv, glv, &gy, row);
    } else {
      for (int j = 0; j < S; ++j) row[j] = 0.f;
    }
    g_in[b * D + col] = gy;
  }
  __syncthreads();
  unstage_rows(gP + b0 * dt * S, sp, n);
}

// ---- ShiftBounds.inverse on the stored bounds (bijectors.py:210-240) ----------
// The end of the inverse pass, thread per row.  s1: the state after
// ShiftBounds (sb == NULL: no ShiftBounds, x is that state); s0: where the
// op's input state goes (may be s1 when sb is NULL).  Per dim
//   BOTH   x = z b + (1 - z) a                 log-det  log(1 / (b - a))
//   NONE   x = t = z xmax + (1 - z) xmin                log(1 / (xmax - xmin))
//   LOWER  x = exp(t) + a                               log(1 / (xmax - xmin)) - t
//   UPPER  x = b - exp(t)                               the same
// the log-det being the forward's (bijectors.py:186-207) at the inverse's own
// t.  Closes the row: ld[b] becomes the whole chain's log-det, log_q = latent
// log-density + ld (lat: latent_vjp_kernel's value on a zero log-det, so
// finfo.min / max where the density is not finite, fin != 0 where it is:
// those come out as -inf / +inf), mask[b] (in: the dead flag of
// spline_inv_ld_kernel) becomes 1 on rows whose x and log_q are all finite
// and 0 elsewhere, and a dead row's x is NaN.
__global__ void sb_eval_inv_kernel(const float* __restrict__ s1, float* __restrict__ s0, float* __restrict__ x,
                                   const float* __restrict__ sb, float* __restrict__ ld,
                                   const float* __restrict__ lat, const float* __restrict__ fin,
                                   float* __restrict__ mask, float* __restrict__ log_q, int B, int D) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const bool dead = mask[b] != 0.f;
  bool finx = true;
  float lds = 0.f;
  for (int i = 0; i < D; ++i) {
    const float z = s1[(long long)b * D + i];
    float xi = z;
    if (sb) {
      const float* r = sb + 8 * i;
      const int mode = (int)r[0];
      const float a = r[1], bb = r[2];
      if (mode == ZF_SB_BOTH) {
        xi = z * bb + (1.0f - z) * a;
        lds = lds + logf((float)(1.0 / ((double)bb - (double)a)));
      } else {
        const float xmin = r[3], xmax = r[4];
        const float t = z * xmax + (1.0f - z) * xmin;
        const float l = logf(1.0f / (xmax - xmin));
        xi = t;
        if (mode == ZF_SB_LOWER) xi = expf(t) + a;
        if (mode == ZF_SB_UPPER) xi = bb - expf(t);
        lds = lds + (mode == ZF_SB_NONE ? l : l - t);
      }
      s0[(long long)b * D + i] = xi;
    }
    finx = finx && finitef(xi);
    x[(long long)b * D + i] = dead ? __builtin_nanf("") : xi;
  }
  const float ldt = ld[b] + lds;
  ld[b] = ldt;
  const float la = lat[b];
  const float lq = (fin[b] != 0.f ? la : (la > 0.f ? INFINITY : -INFINITY)) + ldt;
  if (log_q) log_q[b] = lq;
  mask[b] = (!dead && finx && finitef(lq)) ? 1.0f : 0.f;
}

// Its reverse, the start of the reverse pass: g = d L / d s1 from gx = d L / d x
// and the row's d L / d log_q (ce, already masked), element per thread:
//   BOTH  gx (b - a)            NONE  gx (xmax - xmin)
//   LOWER (gx exp(t) - ce) (xmax - xmin)      UPPER (-gx exp(t) - ce) (xmax - xmin)
// (sb == NULL: g = gx).  Masked rows are written as zeros.
__global__ void sb_eval_inv_bwd_kernel(const float* __restrict__ s1, const float* __restrict__ gx,
                                       const float* __restrict__ ce, const float* __restrict__ mask,
                                       const float* __restrict__ sb, float* __restrict__ g, int B, int D) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)B * D) return;
  const long long b = e / D;
  const int i = (int)(e - b * D);
  float out = gx[e];
  if (sb) {
    const float* r = sb + 8 * i;
    const int mode = (int)r[0];
    const float a = r[1], bb = r[2];
    if (mode == ZF_SB_BOTH) {
      out = out * (float)((double)bb - (double)a);
    } else {
      const float xmin = r[3], xmax = r[4], z = s1[e];
      const float w = xmax - xmin;
      if (mode != ZF_SB_NONE) {
        const float et = expf(z * xmax + (1.0f - z) * xmin);
        out = (mode == ZF_SB_LOWER ? out * et : -out * et) - ce[b];
      }
      out = out * w;
    }
  }
  g[e] = mask[b] == 0.f ? 0.f : out;
}

// ---- row kernels of the pass ---------------------------------------------------
// The latent rows into the last state: logical dim j is column pmod(j + rot, D)
// (Roll is an index rotation in the trainer's states).
__global__ void rot_in_kernel(const float* __restrict__ z, float* __restrict__ s, int B, int D, int rot) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)B * D) return;
  const long long b = e / D;
  const int j = (int)(e - b * D);
  s[b * D + pmodi(j + rot, D)] = z[e];
}

// ce[b] = d L / d log_q of a row that counts: glq[b] (NULL: 0) where mask[b] != 0.
// glq may be ce itself (in place).
__global__ void mask_cot_kernel(const float* glq, const float* __restrict__ mask, float* ce, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  ce[b] = (glq && mask[b] != 0.f) ? glq[b] : 0.f;
}

// gz = d L / d z: the chain's cotangent on the last state plus the latent's
// (gl: latent_vjp_kernel's ce . d log pi / dz, NULL without a log_q
// cotangent), back in logical dim order; zero rows where mask is 0.
__global__ void gz_out_kernel(const float* __restrict__ g, const float* __restrict__ gl,
                              const float* __restrict__ mask, float* __restrict__ gz, int B, int D, int rot) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)B * D) return;
  const long long b = e / D;
  const int j = (int)(e - b * D);
  const long long src = b * D + pmodi(j + rot, D);
  gz[e] = mask[b] == 0.f ? 0.f : (gl ? g[src] + gl[src] : g[src]);
}

}  // namespace
}  // namespace zf
