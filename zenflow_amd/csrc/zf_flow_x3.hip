// Host side of the split-MFMA fused flow kernel (zf_flow_x3_kernel.h): which
// calls take the resident form, and the launch dispatch to the per-knot-count
// translation units zf_flow_x3_k{8,16,32,64}.hip.  What the kernels read is
// packed by zf_flow_image.hip (x3_eligible, x3_pack).
#include "zf_flow_x3_kernel.h"

#include <cstdlib>

namespace zf {

int launch_x3_k8(const X3Launch& a, bool inverse);
int launch_x3_k16(const X3Launch& a, bool inverse);
int launch_x3_k32(const X3Launch& a, bool inverse);
int launch_x3_k64(const X3Launch& a, bool inverse);

// ZF_X3_RESIDENT, read by zf_flow_create: 0 = never the resident
// form (flow_kernel_x3r), 1 = whenever the call is eligible, anything else
// (unset) = automatic, from the measured row count on (zf_flow.hip).
int x3_resident_mode() {
  const char* env = std::getenv("ZF_X3_RESIDENT");
  if (env && env[0] == '0' && env[1] == 0) return 0;
  if (env && env[0] == '1' && env[1] == 0) return 1;
  return -1;
}

// Whether this call can run the resident form on `ncu` CUs, one block each:
// f16x2 swish at hidden 128 with one streamed hidden layer per coupling and
// one pair of transformed dims, an NSC in the op range, an instantiated
// kernel, and the LDS budget: the largest coupling's whole span + one
// parameter region + 12 waves x 2 state buffers + one fp64 sum per tile of
// the block <= 160 KiB.  With T = 4: span = 4 x 16 KiB + 4 x TL x 4 KiB
// (112 KiB at K = 16, two dims), so K = 32 with two dims (160 KiB) never fits.
bool x3_resident_fits(const zf_flow_desc& desc, X3Launch& a, bool inverse, int ncu) {
  if (a.NT != 2 || a.T != 4 || a.oact || ncu <= 0 || a.N <= 0) return false;
  const int dt = desc.dim / 2;
  if (dt > 2) return false;  // a dim-pair loop (PAIRS)
  bool in_range = false;
  for (int i = 0; i < desc.n_ops; ++i) {
    if (desc.ops[i].kind != ZF_OP_NSC) continue;
    if (desc.ops[i].n_hidden != 2) return false;
    if (i >= a.op_begin && i < a.op_end) in_range = true;
  }
  if (!in_range) return false;
  const int TL = x3_last_tiles(dt, a.K);
  const long long span = 4ll * (2 * 4 * 2 * 1024) + 4ll * (2 * TL * 2 * 1024);
  const long long nslots = (a.N + 127) / 128;
  const long long slots = (nslots + ncu - 1) / ncu;
  if (slots > (1 << 20)) return false;
  if (x3_res_lds_bytes((size_t)span, a.par_bytes, a.D + a.C, 4 * slots, false) > 160 * 1024) return false;
  // instantiated: K = 16 with two transformed dims, forward and inverse
  // (zf_flow_x3_k16_res.hip).  One transformed dim (cfg4's shape) fits the
  // budget too but did not beat the streaming form by the A/B margin
  // (profiles/resident_ab.txt), and K = 8 / 32 were not measured.
  if (a.K != 16 || dt != 2) return false;
  // The specialised frame (flow_kernel_x3r FR): the flagship shape — D = 4,
  // C = 0, affine ShiftBounds rows only, a Normal latent, no log_det_in —
  // with at most one ShiftBounds in each run of ops between two couplings
  // (the frame keeps one set of its constants before and one behind the
  // pass's coupling).  Its coupling body is compiled for that shape alone
  // (x3_nsc LIT, X3Lit): dt = dc = DC = 2 and one layer-0 k-step follow from
  // D = 4 and C = 0, one streamed hidden layer and swish are required above,
  // and here: every coupling of the op range has exactly K real knots (no
  // padded or mixed knot counts) and its small parameters at X3Lit's offsets
  // (par_lit).  Everything else keeps the generic frame.
  a.res_frame = a.D == 4 && a.C == 0 && a.sb_affine && a.latent == ZF_LATENT_NORMAL &&
                a.ld_in == nullptr && a.par_lit;
  for (int i = a.op_begin, run = 0; i < a.op_end && a.res_frame; ++i) {
    const int kind = desc.ops[i].kind;
    if (kind == ZF_OP_NSC && desc.ops[i].knots != a.K) a.res_frame = false;
    run = kind == ZF_OP_NSC ? 0 : run + (kind == ZF_OP_SHIFT_BOUNDS ? 1 : 0);
    if (run > 1) a.res_frame = false;
  }
  // the frame's ShiftBounds constants take 128 B of LDS more: a call that only fits without them keeps the generic frame
  if (x3_res_lds_bytes((size_t)span, a.par_bytes, a.D + a.C, 4 * slots, true) > 160 * 1024) a.res_frame = false;
  a.res_blocks = ncu;
  a.res_slots = (int)slots;
  a.res_span = (int)span;
  return true;
}

int launch_flow_x3(const X3Launch& a, bool inverse) {
  if (a.NT != 2 && a.NT != 3) return einval("split-MFMA kernel: scheme %d", a.NT);
  if (a.K == 8) return launch_x3_k8(a, inverse);
  if (a.K == 16) return launch_x3_k16(a, inverse);
  if (a.K == 32) return launch_x3_k32(a, inverse);
  if (a.K == 64) return launch_x3_k64(a, inverse);
  return enotsup("split-MFMA kernel: knots not instantiated");
}

}  // namespace zf
