// The flow image (zf_flow_image.hip): everything the eval kernels and their
// launcher read of a flow, built on the host from (zf_flow_desc, natural blob,
// options) by one pure function — no kernel, no HIP call, no environment.
// The device descriptor's types live here so that the image unit (and a
// host-only program that checks it) needs no kernel header.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/zenflow_amd.h"

namespace zf {

constexpr int kMaxOps = 64;
constexpr int kX3Waves = 4;  // split-MFMA kernels: waves per block, 32 samples each
// f16x2 split-MFMA kernels: a swished layer's weights and bias carry log2(e)
// (x3_pack), so its activation is v * rcp(1 + exp2(-v)) without the multiply
constexpr float kSwishPrescale = 1.44269504088896341f;

struct DevOp {
  int kind, shift, K, S;
  int n_hidden, dt, dc, DC;
  int KS0, T_last, nslot_mask, act;
  long long w[17];
  long long b[17];
  long long bn;
  long long sb;
  long long first_chunk;  // blob offset of this NSC's first streamed weight chunk (fp32 kernel)
  // bf16x3 kernel: byte offset of this NSC's weight-group stream in the x3
  // blob, its group count, blob offset of the row-permuted last-layer bias,
  // and the next NSC op index in forward / inverse execution order (or -1).
  long long x3;
  long long x3_blast;
  int x3_groups, x3_tlast;
  int x3_next[2];
  int x3_kw[17];  // f16x2: power-of-two weight scale of streamed layer l (1..n_hidden)
  // f16x2 swish: per Dense_l (0..n_hidden-1, as packed: log2(e) prescale
  // included) R = max_j sum_k |W[k][j]| and B = max_j |b[j]|, so every
  // pre-activation |v_j| <= R * max_k |a_k| + B (x3_early_scale)
  float x3_rb[16][2];
  // split-MFMA kernel: this NSC's small parameters (BatchNorm, Dense_0,
  // biases, the permuted last bias) are the contiguous blob floats
  // [bn, bn + 256 * x3_par_pieces), DMA'd into LDS one NSC ahead
  int x3_par_pieces;
  // the next NSC in forward / inverse execution order (x3_next[d] >= 0):
  // its group-0 byte offset and pieces, its parameter block and pieces —
  // copied here so the kernel's per-NSC scalars are one batch of independent loads
  long long x3_nbase[2], x3_nbn[2];
  int x3_npieces[2], x3_npar[2];
};

struct DevFlow {
  int D, C, latent, n_ops;
  int HP, nslot, per_wave, x3_ok;
  int small_floats;  // packed blob [0, small_floats): per-op small parameters
  int x3_par_bytes;  // split-MFMA kernel: LDS bytes of one NSC's small-parameter region (max over NSCs)
  int kreal;  // split-MFMA kernels: the couplings' knot count (the kernel's K may be padded above it)
  int _pad;
  float lat_c0, lat_c1, lat_c2, lat_c3;
  DevOp ops[kMaxOps];
  // softmax_with_threshold's constants of every coupling's K (KnotConsts: c,
  // norm, rnorm, 0), formed on the device once at zf_flow_create
  // (knot_consts_kernel) so that the resident form does not divide in fp64
  // per tile.  Behind the ops: their stride, which every
  // kernel's code holds as a literal, stays what it was.
  float kc[kMaxOps][4];
};

// The coupling as the resident form's specialised frame runs it (x3_nsc LIT):
// D = 4, C = 0 (dt = dc = DC = 2, one layer-0 k-step), hidden 128 with one
// streamed hidden layer, swish, and exactly K real knots.  The shape fixes the
// layout of the small-parameter region (BatchNorm rows, Dense_0, the biases,
// the permuted last bias), so its offsets are literals (float offsets from
// op.bn; build_flow_image checks them against the image's, op_par_lit), and
// what is left of the op's scalars — the layer scales, the bound pairs and the
// knot constants — is read once per pass, not per tile.
struct X3Lit {
  static constexpr int kW0 = 8;                 // Dense_0 fragments, behind the 3 x 2 BatchNorm rows
  static constexpr int kB0 = kW0 + 4 * 64;      // Dense_0's bias; the hidden bias follows it
  static constexpr int blast(int K) { return kB0 + 2 * 128 + (2 * (3 * K - 1) + 31) / 32 * 32; }
  float bc, rnorm;  // KnotConsts: c * rnorm, rnorm (both resident frames carry these two through a pass)
  float rb[2][2];   // DevOp::x3_rb of Dense_0 and Dense_1
  int kw1, kw_last;
};

// What zf_flow_create reads from the environment, once: ZF_DISABLE_X3=1 and
// ZF_X3_SCHEME (3 = bf16x3, 2 = f16x2, the default).
struct FlowImageOptions {
  bool disable_x3 = false;
  int scheme = 2;
};

struct FlowImage {
  DevFlow dev;                 // as uploaded (kc left zero: the device fills it)
  std::vector<float> packed;   // the device blob
  std::vector<uint16_t> x3;    // split-MFMA group stream, empty when unused
  bool layered = false;        // the layered path: only BatchNorm and ShiftBounds rows are packed
  int x3_K = 0;                // split-MFMA kernels: the instantiated knot count (0: unused)
  bool x3_oact = false;        // some coupling's activation is not swish
  int x3_aset = 0;             // X3Launch::aset: which non-swish activations the flow uses
  // per op, fixed at create (true for ops they do not concern): every
  // ShiftBounds row is NONE or BOTH; an NSC's small parameters sit at X3Lit's offsets
  bool op_sb_affine[kMaxOps], op_par_lit[kMaxOps];
};

// `desc` with its natural-blob offsets filled (zf_flow_plan), `natural` of the planned size.
int build_flow_image(const zf_flow_desc& desc, const float* natural, const FlowImageOptions& opt, FlowImage* out);

// New statistics in `natural` (zf_flow_set_bn_stats / zf_flow_set_sb_stats):
// repack op's rows and return the blob floats [off, off + n) to upload.
struct BlobRegion {
  int64_t off, n;
};
BlobRegion repack_bn(const zf_flow_desc& desc, int op, const float* natural, FlowImage* im);
BlobRegion repack_sb(const zf_flow_desc& desc, int op, const float* natural, FlowImage* im);

// Last-layer tiles of one pass of the split-MFMA kernels at K knots and dt
// transformed dims: 16 parameters per dim and tile for a pair of dims, 32 for one.
int x3_last_tiles(int dt, int K);

}  // namespace zf
