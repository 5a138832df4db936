// Stand-alone host check of the flow image (zenflow_amd/csrc/zf_flow_image.hip):
// builds a fixed set of flows that takes every layout branch once, prints a
// 64-bit FNV-1a digest of each image (descriptor, packed blob, split-MFMA
// stream, kernel-family facts) as one JSON object, and holds the per-op
// launch flags to the two loops launch_flow used to run on every call.
// Host only, no GPU: compile with --cuda-host-only together with
// zf_flow_image.hip and zf_runtime.hip (tests/test_flow_image_host.py).
#include "zf_flow_image.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace zf;

namespace {

uint64_t fnv1a(const void* p, size_t n) {
  uint64_t h = 0xcbf29ce484222325ull;
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
  return h;
}

// 64-bit LCG, top 24 bits -> an exact float in [-1, 1)
struct Rng {
  uint64_t s;
  float unit() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((int)(s >> 40) - (1 << 23)) / (float)(1 << 23);
  }
};

struct Case {
  std::string name;
  zf_flow_desc desc;
  std::vector<float> nat;
  FlowImageOptions opt;
};

zf_flow_desc flow(int D, int C, int latent) {
  zf_flow_desc d;
  std::memset(&d, 0, sizeof(d));
  d.dim = D;
  d.cond_dim = C;
  d.latent = latent;
  d.latent_param = 2.0f;
  return d;
}

void add_sb(zf_flow_desc& d) { d.ops[d.n_ops++].kind = ZF_OP_SHIFT_BOUNDS; }

void add_roll(zf_flow_desc& d, int shift) {
  d.ops[d.n_ops].kind = ZF_OP_ROLL;
  d.ops[d.n_ops++].shift = shift;
}

void add_nsc(zf_flow_desc& d, int K, std::vector<int> hidden, int act) {
  zf_op_desc& op = d.ops[d.n_ops++];
  op.kind = ZF_OP_NSC;
  op.knots = K;
  op.n_hidden = (int)hidden.size();
  for (size_t l = 0; l < hidden.size(); ++l) op.hidden[l] = hidden[l];
  op.act = act;
}

// Plan the natural blob and fill it: layer l of op i has weights of magnitude
// 2^(2l + i mod 3 - 6), so the f16x2 layer scales differ; ShiftBounds row j
// takes sb_modes[j mod n] with bounds and ranges whose reciprocals are exact.
Case make(const char* name, zf_flow_desc d, uint64_t seed, std::vector<int> sb_modes = {ZF_SB_NONE, ZF_SB_BOTH},
          FlowImageOptions opt = FlowImageOptions()) {
  Case c;
  c.name = name;
  c.opt = opt;
  int64_t n = 0;
  if (zf_flow_plan(&d, &n) != ZF_OK) {
    std::fprintf(stderr, "%s: plan failed: %s\n", name, zf_last_error());
    std::exit(2);
  }
  c.desc = d;
  c.nat.assign((size_t)n, 0.f);
  Rng g{seed};
  const int DC = d.dim - d.dim / 2 + d.cond_dim;
  for (int i = 0; i < d.n_ops; ++i) {
    const zf_op_desc& op = d.ops[i];
    if (op.kind == ZF_OP_SHIFT_BOUNDS) {
      for (int j = 0; j < d.dim; ++j) {
        float* r = c.nat.data() + op.off_sb + 8 * j;
        r[0] = (float)sb_modes[j % sb_modes.size()];
        r[1] = -1.f - (float)j;
        r[2] = r[1] + 4.f;
        r[3] = -(float)(1 << (j % 3));
        r[4] = r[3] + 8.f;
      }
    } else if (op.kind == ZF_OP_NSC) {
      float* bn = c.nat.data() + op.off_bn;
      for (int k = 0; k < DC; ++k) {
        bn[k] = 0.25f * g.unit();
        bn[DC + k] = 1.0f + 0.5f * g.unit();
        bn[2 * DC + k] = 1.0f + 0.25f * g.unit();
        bn[3 * DC + k] = 0.125f * g.unit();
      }
      int in = DC;
      for (int l = 0; l <= op.n_hidden; ++l) {
        const int out = l < op.n_hidden ? op.hidden[l] : (d.dim / 2) * (3 * op.knots - 1);
        const float mag = std::ldexp(1.0f, 2 * (l % 5) + i % 3 - 6);
        for (int64_t q = 0; q < (int64_t)in * out; ++q) c.nat[op.off_w[l] + q] = mag * g.unit();
        for (int q = 0; q < out; ++q) c.nat[op.off_b[l] + q] = 0.5f * g.unit();
        in = out;
      }
    }
  }
  return c;
}

// ShiftBounds, then `n` couplings (K, hidden, act) with a Roll between them
zf_flow_desc chain(int D, int C, int latent, int n, int K, std::vector<int> hidden, int act) {
  zf_flow_desc d = flow(D, C, latent);
  add_sb(d);
  for (int i = 0; i < n; ++i) {
    if (i) add_roll(d, 1);
    add_nsc(d, K, hidden, act);
  }
  return d;
}

// Every layout branch once.
std::vector<Case> all_cases() {
  const std::vector<int> h128x2 = {128, 128};
  FlowImageOptions bf16x3, no_x3;
  bf16x3.scheme = 3;
  no_x3.disable_x3 = true;
  const std::vector<int> all_modes = {ZF_SB_UPPER, ZF_SB_NONE, ZF_SB_LOWER, ZF_SB_BOTH};

  std::vector<Case> cases;
  // the flagship: D = 4, ShiftBounds + 4 x (K = 16, (128, 128)) with rolls, swish
  cases.push_back(make("flagship", chain(4, 0, ZF_LATENT_NORMAL, 4, 16, h128x2, ZF_ACT_SWISH), 1));
  cases.push_back(make("flagship_lower_row", chain(4, 0, ZF_LATENT_NORMAL, 4, 16, h128x2, ZF_ACT_SWISH), 1,
                       {ZF_SB_NONE, ZF_SB_LOWER, ZF_SB_BOTH}));
  // one transformed dim, no streamed hidden layer, width padded to 128
  cases.push_back(make("d2_k8_h64", chain(2, 0, ZF_LATENT_UNIFORM, 2, 8, {64}, ZF_ACT_SWISH), 2, all_modes));
  // padded knots (10 -> 16), conditions, aset 1
  cases.push_back(make("d5_c3_k10_tanh", chain(5, 3, ZF_LATENT_BETA, 2, 10, {128, 64}, ZF_ACT_TANH), 3, all_modes));
  // two dim pairs with odd dt, K = Kp - 1, the centred bias fold
  cases.push_back(make("d7_k15_sigmoid", chain(7, 0, ZF_LATENT_TRUNCNORM, 2, 15, {96, 128, 32}, ZF_ACT_SIGMOID), 4));
  {  // mixed knots (8, 24 -> Kp = 32) and activations at hidden 256 (T = 8)
    zf_flow_desc d = flow(4, 0, ZF_LATENT_NORMAL);
    add_sb(d);
    add_nsc(d, 8, {256}, ZF_ACT_SWISH);
    add_roll(d, 2);
    add_nsc(d, 24, {256, 256}, ZF_ACT_SOFTPLUS);
    cases.push_back(make("k8_k24_swish_softplus_h256", d, 5));
  }
  cases.push_back(make("flagship_bf16x3", chain(4, 0, ZF_LATENT_NORMAL, 4, 16, h128x2, ZF_ACT_SWISH), 1,
                       {ZF_SB_NONE, ZF_SB_BOTH}, bf16x3));
  cases.push_back(make("no_x3_k4_h32", chain(4, 0, ZF_LATENT_NORMAL, 2, 4, {32}, ZF_ACT_SWISH), 6,
                       {ZF_SB_NONE, ZF_SB_BOTH}, no_x3));
  cases.push_back(make("no_x3_k8_h200", chain(3, 1, ZF_LATENT_NORMAL, 2, 8, {200}, ZF_ACT_RELU), 7,
                       {ZF_SB_NONE, ZF_SB_BOTH}, no_x3));
  {  // a 1-knot coupling keeps the flow on the fp32 kernel
    zf_flow_desc d = flow(4, 0, ZF_LATENT_NORMAL);
    add_sb(d);
    add_nsc(d, 1, {64}, ZF_ACT_SWISH);
    add_roll(d, 1);
    add_nsc(d, 8, {64}, ZF_ACT_SWISH);
    cases.push_back(make("one_knot", d, 8));
  }
  cases.push_back(make("layered_k100", chain(4, 0, ZF_LATENT_NORMAL, 1, 100, {64}, ZF_ACT_SWISH), 9));
  cases.push_back(make("layered_h512", chain(3, 0, ZF_LATENT_NORMAL, 1, 8, {512}, ZF_ACT_SWISH), 10));
  // split-MFMA eligible, but D = 25 at K = 64 needs 164384 B of LDS (> 160 KiB): the fp32 kernel, HP and blast slots kept
  cases.push_back(make("x3_over_lds_d25_k64_h128", chain(25, 0, ZF_LATENT_NORMAL, 1, 64, {128}, ZF_ACT_SWISH), 11));
  return cases;
}

// The flagship with new BatchNorm statistics for op 3 and new ShiftBounds ranges for op 0.
Case with_new_stats(Case c) {
  c.name = "flagship_repacked";
  const zf_op_desc& nsc = c.desc.ops[3];
  for (int k = 0; k < 2; ++k) {
    c.nat[nsc.off_bn + k] = 0.375f - 0.25f * k;
    c.nat[nsc.off_bn + 2 + k] = 0.75f + 0.5f * k;
  }
  for (int j = 0; j < 4; ++j) {
    c.nat[c.desc.ops[0].off_sb + 8 * j + 3] = -3.f + (float)j;
    c.nat[c.desc.ops[0].off_sb + 8 * j + 4] = 1.f + (float)j;
  }
  return c;
}

// The two loops launch_flow ran on every call before the image carried the
// per-op flags: kept here as the independent statement of what they mean.
bool sb_affine_loop(const zf_flow_desc& desc, const FlowImage& im, int op_begin, int op_end) {
  bool affine = true;
  for (int i = op_begin; i < op_end; ++i) {
    if (desc.ops[i].kind != ZF_OP_SHIFT_BOUNDS) continue;
    for (int j = 0; j < im.dev.D; ++j) {
      const int mode = (int)im.packed[(size_t)im.dev.ops[i].sb + 8 * j];
      if (mode != ZF_SB_NONE && mode != ZF_SB_BOTH) affine = false;
    }
  }
  return affine;
}

bool par_lit_loop(const FlowImage& im, int op_begin, int op_end) {
  bool lit = true;
  for (int i = op_begin; i < op_end; ++i) {
    const DevOp& d = im.dev.ops[i];
    if (d.kind != ZF_OP_NSC) continue;
    if (d.w[0] - d.bn != X3Lit::kW0 || d.b[0] - d.bn != X3Lit::kB0 || d.b[1] - d.b[0] != 128 ||
        d.x3_blast - d.bn != X3Lit::blast(im.x3_K))
      lit = false;
  }
  return lit;
}

int failures = 0;

void expect(bool ok, const std::string& name, const char* what) {
  if (ok) return;
  std::fprintf(stderr, "%s: %s\n", name.c_str(), what);
  ++failures;
}

bool flag_and(const bool* f, int b, int e) {
  bool v = true;
  for (int i = b; i < e; ++i) v = v && f[i];
  return v;
}

// every op range's flags against the loops (par_lit is asked of split-MFMA flows only, as launch_flow did)
void check_flags(const Case& c, const FlowImage& im) {
  const int n = c.desc.n_ops;
  for (int b = 0; b <= n; ++b)
    for (int e = b; e <= n; ++e) {
      expect(flag_and(im.op_sb_affine, b, e) == sb_affine_loop(c.desc, im, b, e), c.name, "sb_affine differs from the loop");
      if (im.dev.x3_ok) expect(flag_and(im.op_par_lit, b, e) == par_lit_loop(im, b, e), c.name, "par_lit differs from the loop");
    }
}

bool first = true;

void report(const Case& c, const FlowImage& im) {
  DevFlow dev = im.dev;  // the latent constants go through libm: not part of the digest
  dev.lat_c0 = dev.lat_c1 = dev.lat_c2 = dev.lat_c3 = 0.f;
  const int facts[6] = {im.layered ? 1 : 0, dev.x3_ok, im.x3_K, im.x3_oact ? 1 : 0, im.x3_aset, dev.HP};
  const int n = c.desc.n_ops;
  std::printf("%s\n  \"%s\": {\"dev\": \"%016llx\", \"packed\": \"%016llx\", \"stream\": \"%016llx\", \"facts\": \"%016llx\","
              " \"layered\": %d, \"x3_ok\": %d, \"x3_K\": %d, \"oact\": %d, \"aset\": %d, \"HP\": %d,"
              " \"sb_affine\": [%d, %d], \"par_lit\": %d}",
              first ? "{" : ",", c.name.c_str(), (unsigned long long)fnv1a(&dev, sizeof(dev)),
              (unsigned long long)fnv1a(im.packed.data(), im.packed.size() * sizeof(float)),
              (unsigned long long)fnv1a(im.x3.data(), im.x3.size() * sizeof(uint16_t)),
              (unsigned long long)fnv1a(facts, sizeof(facts)), facts[0], facts[1], facts[2], facts[3], facts[4], facts[5],
              (int)flag_and(im.op_sb_affine, 0, n), (int)flag_and(im.op_sb_affine, 1, n),
              (int)(dev.x3_ok != 0 && flag_and(im.op_par_lit, 0, n)));
  first = false;
}

FlowImage build(const Case& c) {
  FlowImage im;
  if (build_flow_image(c.desc, c.nat.data(), c.opt, &im) != ZF_OK) {
    std::fprintf(stderr, "%s: build_flow_image failed: %s\n", c.name.c_str(), zf_last_error());
    std::exit(2);
  }
  check_flags(c, im);
  return im;
}

}  // namespace

int main() {
  const std::vector<Case> cases = all_cases();
  for (const Case& c : cases) {
    const FlowImage im = build(c);
    report(c, im);
    const int n = c.desc.n_ops;
    if (c.name == "flagship")
      expect(im.dev.x3_ok == 2 && flag_and(im.op_par_lit, 0, n) && flag_and(im.op_sb_affine, 0, n), c.name,
             "expected f16x2 with par_lit and sb_affine");
    if (c.name == "flagship_lower_row")
      expect(!flag_and(im.op_sb_affine, 0, n) && flag_and(im.op_sb_affine, 1, n), c.name,
             "expected sb_affine false on the full range and true behind op 0");
    if (c.name == "x3_over_lds_d25_k64_h128")
      expect(im.dev.x3_ok == 0 && !im.layered && im.dev.HP == 128 && im.dev.ops[1].x3_blast > 0 && im.x3.empty(), c.name,
             "expected the fp32 kernel with the split-MFMA layout's padding");
  }

  {  // new statistics on the flagship: equal to building the image from the updated natural blob
    FlowImage im = build(cases[0]);
    const Case c = with_new_stats(cases[0]);
    repack_bn(c.desc, 3, c.nat.data(), &im);
    repack_sb(c.desc, 0, c.nat.data(), &im);
    check_flags(c, im);
    report(c, im);
    const FlowImage fresh = build(c);
    expect(fresh.packed == im.packed, c.name, "repacked blob differs from a fresh image of the same parameters");
  }
  std::printf("\n}\n");
  return failures ? 1 : 0;
}
