// The flow image: (zf_flow_desc, natural blob, options) -> the bytes every
// eval kernel reads and the facts the launcher needs (zf_flow_image.h).  Host
// code only: validation and the natural-blob plan, the kernel family, the
// packed blob's layout, the fp32 MFMA fragment order, the split-MFMA group
// stream.  Layouts: zf_flow.hip / zf_flow_x3_kernel.h headers + DESIGN.md
// §Data layout.  Links against zf_runtime.hip alone (set_error).
#include "zf_flow_image.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "zf_internal.h"

namespace zf {
namespace {

int64_t round_up64(int64_t a, int64_t m) { return (a + m - 1) / m * m; }

int next_pow2(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

struct OpGeom {
  int dt, dc, DC, K, S, OUT, KS0, T_last, nslot;
};

OpGeom nsc_geom(const zf_flow_desc& desc, const zf_op_desc& op) {
  OpGeom g;
  const int D = desc.dim;
  g.dt = D / 2;
  g.dc = D - g.dt;
  g.DC = g.dc + desc.cond_dim;
  g.K = op.knots;
  g.S = 3 * g.K - 1;
  g.OUT = g.dt * g.S;
  g.KS0 = (g.DC + 1) / 2;
  g.T_last = (g.OUT + 31) / 32;
  const int span = (g.dt >= 2 ? 2 * g.S : g.S);
  int need = (span + 31) / 32 + 1;
  if (need > g.T_last) need = g.T_last;
  g.nslot = next_pow2(need);
  return g;
}

// Widths up to 256 run in the fused kernels; wider ones on the layered path
// (zf_layered.hip), whose row chunks shrink as the width grows.
constexpr int kMaxFusedWidth = 256, kMaxLayeredWidth = 4096;
// knots: the fused kernels take up to 64 (the split-MFMA kernel's largest
// instantiation, and the fp32 kernel's LDS ring), the layered path's
// per-(row, dim) spline kernels (one row's 3K - 1 parameters per thread in
// LDS) up to 200
constexpr int kMaxFusedKnots = 64, kMaxLayeredKnots = 200;

int validate(const zf_flow_desc* desc) {
  if (!desc) return einval("desc is NULL");
  if (desc->dim < 1 || desc->dim > 64) return einval("dim %d out of range [1, 64]", desc->dim);
  if (desc->cond_dim < 0 || desc->cond_dim > 64) return einval("cond_dim out of range");
  if (desc->n_ops < 0 || desc->n_ops > kMaxOps) return einval("n_ops out of range");
  if (desc->latent < ZF_LATENT_NONE || desc->latent > ZF_LATENT_UNIFORM) return einval("bad latent");
  for (int i = 0; i < desc->n_ops; ++i) {
    const zf_op_desc& op = desc->ops[i];
    if (op.kind == ZF_OP_NSC) {
      if (desc->dim < 2) return einval("NeuralSplineCoupling needs dim >= 2");
      if (op.knots < 1 || op.knots > kMaxLayeredKnots)
        return einval("knots %d out of range [1, %d]", op.knots, kMaxLayeredKnots);
      if (op.n_hidden < 1 || op.n_hidden > 16) return enotsup("n_hidden must be in [1, 16]");
      for (int l = 0; l < op.n_hidden; ++l)
        if (op.hidden[l] < 1 || op.hidden[l] > kMaxLayeredWidth)
          return enotsup("hidden width must be in [1, 4096]");
      if (op.act < 0 || op.act >= ZF_ACT_COUNT) return einval("op %d: unknown activation %d", i, op.act);
    } else if (op.kind != ZF_OP_ROLL && op.kind != ZF_OP_SHIFT_BOUNDS) {
      return einval("op %d: unknown kind %d", i, op.kind);
    }
  }
  return ZF_OK;
}

// What one pass over the ops tells of the flow's couplings.
struct NscScan {
  int hmax = 0, kmax = 0, kmin = 1 << 30;  // widest hidden layer, most and fewest knots
  int klast = 0;           // the last coupling's knots (DevFlow::kreal)
  bool oact = false;       // some activation is not swish
  int aset = 1;            // X3Launch::aset of the non-swish ones: 2 sigmoid / softplus only, 1 the others only, 0 both
};

NscScan scan_nscs(const zf_flow_desc& desc) {
  NscScan s;
  bool centred = false, plain = false;
  for (int i = 0; i < desc.n_ops; ++i) {
    const zf_op_desc& op = desc.ops[i];
    if (op.kind != ZF_OP_NSC) continue;
    for (int l = 0; l < op.n_hidden; ++l) s.hmax = op.hidden[l] > s.hmax ? op.hidden[l] : s.hmax;
    s.kmax = op.knots > s.kmax ? op.knots : s.kmax;
    s.kmin = op.knots < s.kmin ? op.knots : s.kmin;
    s.klast = op.knots;
    if (op.act == ZF_ACT_SWISH) continue;
    s.oact = true;
    if (op.act == ZF_ACT_SIGMOID || op.act == ZF_ACT_SOFTPLUS) centred = true;
    else plain = true;
  }
  s.aset = centred && plain ? 0 : centred ? 2 : 1;
  return s;
}

int hidden_pad_of(int hmax) {
  int hp = 32;
  while (hp < hmax) hp <<= 1;  // instantiated tile counts: 1, 2, 4, 8
  return hp;
}

void pack_nsc_bn(const zf_flow_desc& desc, const zf_op_desc& op, const float* nat, float* dst) {
  const OpGeom g = nsc_geom(desc, op);
  const int DCp = 2 * g.KS0;
  const float* mean = nat + op.off_bn;
  const float* var = mean + g.DC;
  const float* scale = var + g.DC;
  const float* bias = scale + g.DC;
  for (int k = 0; k < DCp; ++k) {
    if (k < g.DC) {
      // flax BatchNorm: mul = rsqrt(var + eps) * scale
      const float mul = (1.0f / std::sqrt(var[k] + 1e-5f)) * scale[k];
      dst[k] = mean[k];
      dst[DCp + k] = mul;
      dst[2 * DCp + k] = bias[k];
    } else {
      dst[k] = dst[DCp + k] = dst[2 * DCp + k] = 0.f;
    }
  }
}

// Returns whether every row is affine (mode NONE or BOTH).
bool pack_sb(const zf_flow_desc& desc, const zf_op_desc& op, const float* nat, float* dst) {
  bool affine = true;
  for (int i = 0; i < desc.dim; ++i) {
    const float* r = nat + op.off_sb + 8 * i;
    const int mode = (int)r[0];
    const float a = r[1], b = r[2], xmin = r[3], xmax = r[4];
    float mul;
    if (mode == ZF_SB_BOTH) mul = (float)(1.0 / ((double)b - (double)a));  // :189 (Python floats)
    else mul = 1.0f / (xmax - xmin);                                        // :265
    float* o = dst + 8 * i;
    o[0] = (float)mode; o[1] = a; o[2] = b; o[3] = xmin; o[4] = xmax;
    o[5] = mul; o[6] = std::log(mul); o[7] = 0.f;
    if (mode != ZF_SB_NONE && mode != ZF_SB_BOTH) affine = false;
  }
  return affine;
}

// Unit row of accumulator register r in lane half hh of 32-row output tile o
// (v_mfma_f32_32x32: four rows, then a stride of eight); a bias tile is
// packed in that order, [tile][lane half][16].
int acc_row(int o, int hh, int r) { return 32 * o + (r & 3) + 8 * (r >> 2) + 4 * hh; }

void pack_bias_tiles(const float* B, int out, int tiles, float* dst) {
  for (int o = 0; o < tiles; ++o)
    for (int hh = 0; hh < 2; ++hh)
      for (int r = 0; r < 16; ++r) {
        const int ii = acc_row(o, hh, r);
        dst[(o * 2 + hh) * 16 + r] = ii < out ? B[ii] : 0.f;
      }
}

// Dense_l of one coupling in fp32 MFMA A-fragment order, zero beyond (in, out):
//   layer 0, fragment (o, ks): lane -> W[k = 2ks + (lane>>5)][i = 32o + (lane&31)]
//   layers 1..n_hidden, fragment (o, t, r4, lane, e) -> W[k = 32t + e + 8 r4 + 4 (lane>>5)][i = 32o + (lane&31)]
// and its bias tiles.
void pack_fp32_layer(const zf_op_desc& op, const OpGeom& g, const DevOp& d, int l, int T, const float* nat, float* P) {
  const int in = l == 0 ? g.DC : op.hidden[l - 1];
  const int out = l < op.n_hidden ? op.hidden[l] : g.OUT;
  const int To = l < op.n_hidden ? T : g.T_last;
  const float* W = nat + op.off_w[l];
  auto w = [&](int k, int ii) { return (k < in && ii < out) ? W[(int64_t)k * out + ii] : 0.f; };
  float* Wp = P + d.w[l];
  for (int o = 0; o < To; ++o)
    if (l == 0) {
      for (int ks = 0; ks < g.KS0; ++ks)
        for (int ln = 0; ln < 64; ++ln) Wp[((int64_t)o * g.KS0 + ks) * 64 + ln] = w(2 * ks + (ln >> 5), 32 * o + (ln & 31));
    } else {
      for (int t = 0; t < T; ++t)
        for (int r4 = 0; r4 < 4; ++r4)
          for (int ln = 0; ln < 64; ++ln)
            for (int e = 0; e < 4; ++e)
              Wp[((((int64_t)o * T + t) * 4 + r4) * 64 + ln) * 4 + e] =
                  w(32 * t + e + 8 * r4 + 4 * (ln >> 5), 32 * o + (ln & 31));
    }
  pack_bias_tiles(nat + op.off_b[l], out, To, P + d.b[l]);
}

// Split-MFMA kernels (zf_flow_x3_kernel.h).

uint16_t bf16_rne(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // quiet NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

float bf16_f(uint16_t b) {
  const uint32_t u = (uint32_t)b << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

int x3_last_tiles_pair(int K) { return (3 * K - 1 + 15) / 16; }
// ONE layout (one transformed dim): 32 parameters per tile
int x3_last_tiles_one(int K) { return (3 * K - 1 + 31) / 32; }

int x3_pairs(const zf_flow_desc& desc) { return (desc.dim / 2 + 1) / 2; }

// The instantiated knot count a flow of K knots runs at (0: none).  K < Kp
// runs as Kp knots whose extra ones are inert (x3_param_of): their widths /
// heights enter the sums as exact zeros (logit -2^40: squareplus = 0) and
// their slope logits are 0 at the last real knot (the boundary derivative
// 1) and NaN beyond, so the idx == K sliver still gives NaN (utils.py:
// 224-230).  K = Kp - 1 has no NaN slope: the kernel starts the sliver at
// knot K itself (rqs_bin_monotone's padlast, per coupling).  K in 33..64
// runs at 64 (one wave per SIMD: 12 last-layer tiles and 191 spline
// parameters per lane, x3_occupancy).
int x3_padded_knots(int K) {
  if (K < 2) return 0;
  if (K <= 8) return 8;
  if (K <= 16) return 16;
  if (K <= 32) return 32;
  if (K <= 64) return 64;
  return 0;
}

// Parameter jp (of 3 Kp - 1) of a padded (sample, dim) row -> the real
// parameter of 3 K - 1 (widths, heights, slopes), or -1 with the inert
// value in *fill.
int x3_param_of(int jp, int Kp, int K, float* fill) {
  if (jp < Kp) {
    *fill = -1099511627776.0f;  // -2^40: x + sqrt(x^2 + 4) = 0 exactly
    return jp < K ? jp : -1;
  }
  if (jp < 2 * Kp) {
    *fill = -1099511627776.0f;
    return jp - Kp < K ? K + (jp - Kp) : -1;
  }
  const int q = jp - 2 * Kp;
  *fill = q == K - 1 ? 0.0f : __builtin_nanf("");
  return q < K - 1 ? 2 * K + q : -1;
}

// The instantiated knot count all couplings run the split-MFMA kernels at —
// the largest one's, as a chain may mix knot counts — or 0: not eligible.
// Hidden <= 128 runs padded to 128 (the caller pads HP); any dim the fp32
// kernel takes (LDS is checked by the caller).
int x3_eligible(const NscScan& scan, int HP, const FlowImageOptions& opt) {
  if (opt.disable_x3 || HP > 256) return 0;
  // relu, leaky_relu, tanh, gelu and elu (act(0) = 0, |act(v)| <= |v|: the
  // f16x2 per-sample power-of-two scale keeps every value's relative
  // precision) run on f16x2 as they are; sigmoid and softplus run centred
  // (act(v) - C, C = 1/2 / log 2 folded into the next bias: act_tile_centered,
  // x3_pack).  bf16x3 (the scaling-free reference scheme) is instantiated for
  // swish couplings only: its activation-switch builds were 10 MB of the
  // library for an opt-in scheme, so other activations there run the fp32
  // kernel (softplus had to anyway: in the tiny-activation
  // regime bf16x3's mean error was 5x the fp32 oracle's,
  // profiles/r03_diag_acts.jsonl, held by
  // tests/test_gpu_flow.py::test_split_scaling_extremes_other_acts).
  if (scan.oact && opt.scheme == 3) return 0;
  // a 1-knot coupling anywhere keeps the flow off these kernels, as a flow of
  // 1-knot couplings is (that case is not pinned)
  return scan.kmin < 2 ? 0 : x3_padded_knots(scan.kmax);
}

// Weight-buffer tiles: the larger of a hidden group (T) and a last-layer
// group (x3_last_tiles, one pass of the last layer).
int x3_buf_tiles(const zf_flow_desc& desc, int T, int K) { return std::max(T, x3_last_tiles(desc.dim / 2, K)); }

// TB = x3_buf_tiles; D = dim + cond_dim (the per-wave state holds x and c);
// par_bytes = DevFlow::x3_par_bytes
size_t x3_lds_bytes(int TB, int D, int NT, int par_bytes) {
  return (size_t)2 * 2 * TB * NT * 1024 + (size_t)2 * par_bytes + (size_t)kX3Waves * 32 * D * 4 +
         kX3Waves * sizeof(double);
}

// Pack the group streams (bf16 hi/mid/lo or f16 hi/lo A fragments) of every
// NSC and the row-permuted last-layer biases (into the blob at
// ops[i].x3_blast), and turn the image over to the split-MFMA kernels of
// scheme NT at Kp knots.
void x3_pack(const zf_flow_desc& desc, const float* nat, int T, int NT, int Kp, const NscScan& scan, FlowImage& im) {
  DevFlow& F = im.dev;
  float* packed = im.packed.data();
  std::vector<uint16_t>& stream = im.x3;
  F.x3_ok = NT == 3 ? 1 : 2;
  F.kreal = scan.klast;
  im.x3_K = Kp;
  im.x3_oact = scan.oact;
  im.x3_aset = scan.aset;
  int prev = -1;
  for (int i = 0; i < desc.n_ops; ++i) {
    F.ops[i].x3_next[0] = F.ops[i].x3_next[1] = -1;
    if (desc.ops[i].kind != ZF_OP_NSC) continue;
    if (prev >= 0) { F.ops[prev].x3_next[0] = i; F.ops[i].x3_next[1] = prev; }
    prev = i;
  }
  for (int i = 0; i < desc.n_ops; ++i) {
    const zf_op_desc& op = desc.ops[i];
    if (op.kind != ZF_OP_NSC) continue;
    DevOp& d = F.ops[i];
    // K: the coupling's knots; Kp: the instantiation's (x3_padded_knots)
    const int dt = desc.dim / 2, K = Kp, S = 3 * K - 1;  // every coupling at the flow's instantiation
    const int Kr = op.knots, Sr = 3 * Kr - 1;
    const bool one = dt == 1;
    const int TL = x3_last_tiles(dt, K), NP = x3_pairs(desc);
    // Last layer, pair pr, tile o, lane half h, row r: the padded parameter jp
    // of transformed dim dd -> its column of the natural layer, or -1 with
    // *fill what an inert padding knot takes (0 outside the padded row)
    auto last_col = [&](int pr, int o, int h, int r, float* fill) {
      const int jp = one ? 32 * o + 16 * h + r : 16 * o + r, dd = one ? 0 : 2 * pr + h;
      *fill = 0.f;
      const int jr = (dd < dt && jp < S) ? x3_param_of(jp, K, Kr, fill) : -1;
      return jr >= 0 ? dd * Sr + jr : -1;
    };
    d.x3 = (long long)stream.size() * 2;
    d.x3_tlast = TL;
    d.x3_groups = T * (op.n_hidden - 1) + T * NP;
    for (int l = 1; l <= op.n_hidden; ++l) {
      const bool last = (l == op.n_hidden);
      const int in = op.hidden[l - 1];
      const int out = last ? dt * Sr : op.hidden[l];
      const int NOUT = last ? TL : T;
      const float* W = nat + op.off_w[l];
      // f16x2: the inputs of swished layers' activations carry log2(e)
      const float pre = (NT == 2 && !last && op.act == ZF_ACT_SWISH) ? kSwishPrescale : 1.0f;
      // f16x2: the layer's power-of-two scale, max |W| * 2^kw in [2^13, 2^14)
      int kw = 0;
      if (NT == 2) {
        float mx = 0.f;
        for (int64_t i = 0; i < (int64_t)in * out; ++i)
          mx = std::fmax(mx, std::fabs(W[i] * pre));
        if (mx > 0.f && std::isfinite(mx)) {
          int e;
          std::frexp(mx, &e);
          kw = 14 - e;
        }
      }
      d.x3_kw[l] = kw;
      for (int pr = 0; pr < (last ? NP : 1); ++pr)
        for (int q = 0; q < T; ++q)
          for (int s = 0; s < 2; ++s)
            for (int o = 0; o < NOUT; ++o) {
              uint16_t part[3][64][8];  // [term][lane][element]
              for (int ln = 0; ln < 64; ++ln)
                for (int j = 0; j < 8; ++j) {
                  const int kstep = 2 * q + s;
                  const int k = 16 * kstep + 8 * (j >> 2) + 4 * (ln >> 5) + (j & 3);
                  const int rho = ln & 31;
                  float fill;
                  int col = last ? last_col(pr, o, (rho >> 2) & 1, (rho & 3) + 4 * (rho >> 3), &fill) : 32 * o + rho;
                  if (col >= out) col = -1;
                  const float x = (k < in && col >= 0) ? W[(int64_t)k * out + col] : 0.f;
                  if (NT == 3) {
                    const uint16_t bh = bf16_rne(x);
                    const float r1 = x - bf16_f(bh);
                    const uint16_t bm = bf16_rne(r1);
                    const uint16_t bl = bf16_rne(r1 - bf16_f(bm));
                    part[0][ln][j] = bh;
                    part[1][ln][j] = bm;
                    part[2][ln][j] = bl;
                  } else {
                    const float xs = std::ldexp(x * pre, kw);
                    const _Float16 h = (_Float16)xs;  // RNE
                    const _Float16 lo = (_Float16)(xs - (float)h);
                    std::memcpy(&part[0][ln][j], &h, 2);
                    std::memcpy(&part[1][ln][j], &lo, 2);
                  }
                }
              const uint16_t* pp = &part[0][0][0];
              stream.insert(stream.end(), pp, pp + NT * 64 * 8);
            }
    }
    // f16x2 sigmoid / softplus: the kernel feeds act(v) - C to every layer
    // after Dense_0 (act_tile_centered), so each such layer's bias takes
    // C * sum_k W[k][j] (fp64 sums, rounded once); the last layer's fold goes
    // into the permuted last bias below
    std::vector<double> lastfold;
    if (NT == 2 && (op.act == ZF_ACT_SIGMOID || op.act == ZF_ACT_SOFTPLUS)) {
      const double C = op.act == ZF_ACT_SIGMOID ? 0.5 : 0.69314718055994530942;
      for (int l = 1; l <= op.n_hidden; ++l) {
        const bool last = l == op.n_hidden;
        const int in = op.hidden[l - 1];
        const int out = last ? dt * Sr : op.hidden[l];
        const float* W = nat + op.off_w[l];
        std::vector<double> cs(out, 0.0);
        for (int k = 0; k < in; ++k)
          for (int j = 0; j < out; ++j) cs[j] += (double)W[(int64_t)k * out + j];
        if (last) {
          for (double& v : cs) v *= C;
          lastfold.swap(cs);
          continue;
        }
        for (int o = 0; o < T; ++o)
          for (int hh = 0; hh < 2; ++hh)
            for (int r = 0; r < 16; ++r) {
              const int ii = acc_row(o, hh, r);
              if (ii < out) {
                float& b = packed[d.b[l] + (o * 2 + hh) * 16 + r];
                b = (float)((double)b + C * cs[ii]);
              }
            }
      }
    }
    // f16x2: Dense_0 (fp32 fragments, d.w[0]) and the hidden biases of the
    // swished layers join the log2(e) prescale (act_swish); other
    // activations take their pre-activations unscaled.
    for (int l = 0; l < 16; ++l) d.x3_rb[l][0] = d.x3_rb[l][1] = 0.f;
    if (NT == 2 && op.act == ZF_ACT_SWISH) {
      const int KS0 = d.KS0;
      for (int64_t i = 0; i < (int64_t)T * KS0 * 64; ++i) packed[d.w[0] + i] *= kSwishPrescale;
      for (int l = 0; l < op.n_hidden; ++l)
        for (int64_t i = 0; i < (int64_t)T * 32; ++i) packed[d.b[l] + i] *= kSwishPrescale;
      // the per-layer pre-activation bounds of x3_early_scale (the prescaled
      // weights and biases as the kernel multiplies them; fp64 row sums
      // rounded up by a relative 2^-20, so the float bound holds)
      const double pre = kSwishPrescale;
      for (int l = 0; l < op.n_hidden && l < 16; ++l) {
        const int in = l == 0 ? desc.dim - dt + desc.cond_dim : op.hidden[l - 1];
        const int out = op.hidden[l];
        const float* W = nat + op.off_w[l];
        const float* Bv = nat + op.off_b[l];
        double R = 0.0, Bm = 0.0;
        for (int j = 0; j < out; ++j) {
          double rs = 0.0;
          for (int k = 0; k < in; ++k) rs += std::fabs((double)W[(int64_t)k * out + j]);
          R = std::fmax(R, rs * pre);
          Bm = std::fmax(Bm, std::fabs((double)Bv[j]) * pre);
        }
        d.x3_rb[l][0] = (float)(R * (1.0 + 0x1p-20));
        d.x3_rb[l][1] = (float)(Bm * (1.0 + 0x1p-20));
      }
    }
    // group-0 pieces of this NSC (hidden group, or a last-layer group when it has no hidden streamed layer)
    d.x3_npieces[0] = d.x3_npieces[1] = (2 * (op.n_hidden > 1 ? T : TL) * NT * 1024) >> 10;  // own; fixed below
    // permuted last bias: [pair][o][lane half h][r] = bias[(2 pair + h) S + 16o + r]
    const float* B = nat + op.off_b[op.n_hidden];
    for (int pr = 0; pr < NP; ++pr)
      for (int o = 0; o < TL; ++o)
        for (int h = 0; h < 2; ++h)
          for (int r = 0; r < 16; ++r) {
            float b;
            const int col = last_col(pr, o, h, r, &b);
            if (col >= 0) b = lastfold.empty() ? B[col] : (float)((double)B[col] + lastfold[col]);
            packed[d.x3_blast + ((pr * TL + o) * 2 + h) * 16 + r] = b;
          }
  }
  // next-NSC copies (x3_npieces above held each op's own group-0 pieces)
  std::vector<int> own(desc.n_ops, 0);
  for (int i = 0; i < desc.n_ops; ++i) own[i] = desc.ops[i].kind == ZF_OP_NSC ? F.ops[i].x3_npieces[0] : 0;
  for (int i = 0; i < desc.n_ops; ++i) {
    if (desc.ops[i].kind != ZF_OP_NSC) continue;
    DevOp& d = F.ops[i];
    for (int dir = 0; dir < 2; ++dir) {
      const int n = d.x3_next[dir];
      d.x3_nbase[dir] = n >= 0 ? F.ops[n].x3 : -1;
      d.x3_nbn[dir] = n >= 0 ? F.ops[n].bn : 0;
      d.x3_npieces[dir] = n >= 0 ? own[n] : 0;
      d.x3_npar[dir] = n >= 0 ? F.ops[n].x3_par_pieces : 0;
    }
    im.op_par_lit[i] = d.w[0] - d.bn == X3Lit::kW0 && d.b[0] - d.bn == X3Lit::kB0 && d.b[1] - d.b[0] == 128 &&
                       d.x3_blast - d.bn == X3Lit::blast(Kp);
  }
}

// Latent constants in fp32, as jax.scipy.stats computes them.
void latent_consts(const zf_flow_desc& desc, DevFlow& F) {
  const float s2 = 0.1f * 0.1f;
  F.lat_c0 = std::log(6.28318530717958647692f * s2);
  F.lat_c1 = s2;
  if (desc.latent == ZF_LATENT_BETA) {
    const double a = desc.latent_param;
    F.lat_c0 = (float)(-(std::lgamma(a) + std::lgamma(a) - std::lgamma(2.0 * a)));
    F.lat_c1 = (float)a - 1.0f;
    F.lat_c3 = (float)a;  // peakness, for on-device sampling
  } else if (desc.latent == ZF_LATENT_TRUNCNORM) {
    // _log_gauss_mass(-5, 5) = log1p(-ndtr(-5) - ndtr(-5))
    const float nd = (float)(0.5 * std::erfc(5.0 / std::sqrt(2.0)));
    F.lat_c2 = std::log1p(-nd - nd);
  }
}

// The packed blob's layout into F.ops; returns its floats.  Small per-op
// parameters (ShiftBounds rows, BatchNorm, first Dense, biases) first, for all
// ops: the split-MFMA kernel stages each NSC's in LDS.  The streamed fp32
// weight fragments follow.  x3K != 0: the split-MFMA kernels' permuted last
// bias too — with the two-dim tile count even for one transformed dim, as
// X3Lit::blast has it — and each NSC's small-parameter region.  layered:
// BatchNorm and ShiftBounds rows only (that path reads the natural weights).
int64_t lay_out(const zf_flow_desc& desc, bool layered, int x3K, DevFlow& F) {
  const int T = F.HP / 32;
  int64_t off = 0;
  auto take = [&](int64_t n) { const int64_t o = off; off = round_up64(off + n, 4); return o; };
  int nslot = 1;
  for (int i = 0; i < desc.n_ops; ++i) {
    const zf_op_desc& op = desc.ops[i];
    DevOp& d = F.ops[i];
    d.kind = op.kind;
    d.shift = op.shift;
    if (op.kind == ZF_OP_NSC) {
      const OpGeom g = nsc_geom(desc, op);
      d.K = g.K; d.S = g.S; d.n_hidden = op.n_hidden; d.dt = g.dt; d.dc = g.dc; d.DC = g.DC;
      d.KS0 = g.KS0; d.T_last = g.T_last; d.nslot_mask = g.nslot - 1; d.act = op.act;
      nslot = g.nslot > nslot ? g.nslot : nslot;
      d.bn = take(3 * 2 * g.KS0);
      if (layered) continue;
      d.w[0] = take((int64_t)T * g.KS0 * 64);
      for (int l = 0; l < op.n_hidden; ++l) d.b[l] = take((int64_t)T * 32);
      d.b[op.n_hidden] = take((int64_t)g.T_last * 32);
      d.x3 = -1;
      if (!x3K) continue;
      d.x3_blast = take((int64_t)x3_pairs(desc) * x3_last_tiles_pair(x3K) * 32);
      // [bn, end of the permuted last bias) as whole 1 KiB DMA pieces (the
      // blob allocation carries 1 KiB of slack past its end)
      const int64_t end = d.x3_blast + (int64_t)x3_pairs(desc) * x3_last_tiles(d.dt, x3K) * 32;
      d.x3_par_pieces = (int)((end - d.bn) * 4 + 1023) / 1024;
      F.x3_par_bytes = std::max(F.x3_par_bytes, d.x3_par_pieces * 1024);
    } else if (op.kind == ZF_OP_SHIFT_BOUNDS) {
      d.sb = take(8 * desc.dim);
    }
  }
  F.small_floats = (int)off;
  for (int i = 0; i < desc.n_ops; ++i) {
    const zf_op_desc& op = desc.ops[i];
    DevOp& d = F.ops[i];
    if (op.kind != ZF_OP_NSC || layered) continue;
    for (int l = 1; l < op.n_hidden; ++l) d.w[l] = take((int64_t)T * T * 1024);
    d.w[op.n_hidden] = take((int64_t)d.T_last * T * 1024);
    d.first_chunk = op.n_hidden > 1 ? d.w[1] : d.w[op.n_hidden];
  }
  F.nslot = nslot;
  F.per_wave = 32 * desc.dim + nslot * 1024;
  return off;
}

}  // namespace

int x3_last_tiles(int dt, int K) { return dt == 1 ? x3_last_tiles_one(K) : x3_last_tiles_pair(K); }

int build_flow_image(const zf_flow_desc& desc, const float* nat, const FlowImageOptions& opt, FlowImage* out) {
  if (!out) return einval("image is NULL");
  if (int rc = validate(&desc)) return rc;
  FlowImage& im = *out;
  im = FlowImage();
  DevFlow& F = im.dev;
  std::memset(&F, 0, sizeof(F));
  F.D = desc.dim;
  F.C = desc.cond_dim;
  F.latent = desc.latent;
  F.n_ops = desc.n_ops;
  latent_consts(desc, F);
  // The kernel family.  A conditioner wider than the fused kernels hold, or
  // with more knots, runs layer by layer; the split-MFMA kernels run hidden
  // <= 128 padded to 128 (4 tiles) — a flow that is eligible for them keeps
  // that padding even when it turns out not to fit their LDS budget.
  const NscScan scan = scan_nscs(desc);
  F.HP = hidden_pad_of(scan.hmax);
  im.layered = F.HP > kMaxFusedWidth || scan.kmax > kMaxFusedKnots;
  if (im.layered) F.HP = 32;  // the fused layouts are then not built
  const int x3K = im.layered ? 0 : x3_eligible(scan, F.HP < 128 ? 128 : F.HP, opt);
  if (x3K && F.HP < 128) F.HP = 128;
  const int T = F.HP / 32;

  const int64_t floats = lay_out(desc, im.layered, x3K, F);
  im.packed.assign((size_t)(floats > 0 ? floats : 4), 0.f);
  float* P = im.packed.data();
  for (int i = 0; i < desc.n_ops; ++i) {
    const zf_op_desc& op = desc.ops[i];
    const DevOp& d = F.ops[i];
    im.op_sb_affine[i] = im.op_par_lit[i] = true;
    if (op.kind == ZF_OP_SHIFT_BOUNDS) {
      im.op_sb_affine[i] = pack_sb(desc, op, nat, P + d.sb);
    } else if (op.kind == ZF_OP_NSC) {
      pack_nsc_bn(desc, op, nat, P + d.bn);
      if (im.layered) continue;
      const OpGeom g = nsc_geom(desc, op);
      for (int l = 0; l <= op.n_hidden; ++l) pack_fp32_layer(op, g, d, l, T, nat, P);
    }
  }
  if (x3K) {
    const int NT = opt.scheme == 3 ? 3 : 2;
    if (x3_lds_bytes(x3_buf_tiles(desc, T, x3K), desc.dim + desc.cond_dim, NT, F.x3_par_bytes) <= 160 * 1024)
      x3_pack(desc, nat, T, NT, x3K, scan, im);
  }
  return ZF_OK;
}

BlobRegion repack_bn(const zf_flow_desc& desc, int op, const float* natural, FlowImage* im) {
  const DevOp& d = im->dev.ops[op];
  pack_nsc_bn(desc, desc.ops[op], natural, im->packed.data() + d.bn);
  return {d.bn, 3 * 2 * d.KS0};
}

BlobRegion repack_sb(const zf_flow_desc& desc, int op, const float* natural, FlowImage* im) {
  const DevOp& d = im->dev.ops[op];
  im->op_sb_affine[op] = pack_sb(desc, desc.ops[op], natural, im->packed.data() + d.sb);
  return {d.sb, 8 * desc.dim};
}

}  // namespace zf

extern "C" int zf_flow_plan(zf_flow_desc* desc, int64_t* blob_floats) {
  int rc = zf::validate(desc);
  if (rc) return rc;
  if (!blob_floats) return zf::einval("blob_floats is NULL");
  int64_t off = 0;
  for (int i = 0; i < desc->n_ops; ++i) {
    zf_op_desc& op = desc->ops[i];
    op.off_bn = op.off_sb = 0;
    for (int l = 0; l < 17; ++l) op.off_w[l] = op.off_b[l] = 0;
    if (op.kind == ZF_OP_NSC) {
      const zf::OpGeom g = zf::nsc_geom(*desc, op);
      op.off_bn = off;
      off += 4 * g.DC;
      int in = g.DC;
      for (int l = 0; l <= op.n_hidden; ++l) {
        const int out = l < op.n_hidden ? op.hidden[l] : g.OUT;
        op.off_w[l] = off;
        off += (int64_t)in * out;
        op.off_b[l] = off;
        off += out;
        in = out;
      }
    } else if (op.kind == ZF_OP_SHIFT_BOUNDS) {
      op.off_sb = off;
      off += 8 * desc->dim;
    }
  }
  *blob_floats = off;
  return ZF_OK;
}
