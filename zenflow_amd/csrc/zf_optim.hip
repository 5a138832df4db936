// Optimiser chains on the device: optax.chain of gradient transformations
// (include/zenflow_amd.h, ZF_OPT_* / ZF_SCHED_*; restated from optax's
// published formulas, zenflow_amd/optim.py).  Per step, after the gradient's
// cast (zf_train.hip, chain_update):
//   sumsq_leaf_kernel    only with clip_by_global_norm: fp64 leaves of sum g^2
//   opt_prologue_kernel  one block: norm and clip factor, lr(count), the Adam
//                        bias corrections, count += 1 (the device scalars)
//   chain_update_kernel  one pass over the blob: the stages in registers
// The same three launches in the captured step graph and eagerly.  A
// translation unit of its own: the trainer's kernels (zf_train.hip and the
// headers it includes) stay the code object they were.
#include "zf_optim.h"

namespace zf {
namespace {

// The pairwise tree of zf_reduce.h's lds_tree over 256 LDS doubles (restated:
// this unit must not include a header that defines kernels), all
// threads of the 256-thread block taking part: level s adds element i + s
// into i for i a multiple of 2s.  Result in p[0].
__device__ __forceinline__ void block_tree_256(double* p) {
  for (int s = 1; s < 256; s *= 2) {
    const int i = 2 * s * (int)threadIdx.x;
    if (i + s < 256) p[i] = p[i] + p[i + s];
    __syncthreads();
  }
}

// The (n)adamw counter of zf_train_kernels.h (step_update there): bc[0] = step t
// as int bits, bc[1] = 1 - b1^t, bc[2] = 1 - b1^(t+1), bc[3] = 1 - b2^t, the
// same expressions so that a restored counter has the bits a run reaches.
__global__ void set_count_kernel(float* __restrict__ bc, int count, float b1, float b2) {
  *reinterpret_cast<int*>(bc) = count;
  if (count > 0) {
    const int t = count;
    bc[1] = (float)(1.0 - pow((double)b1, (double)t));
    bc[2] = (float)(1.0 - pow((double)b1, (double)t + 1.0));
    bc[3] = (float)(1.0 - pow((double)b2, (double)t));
  } else {
    bc[1] = bc[2] = bc[3] = 0.f;
  }
}

// leaf[b] = sum of g[i]^2 over the parameter entries of span b, in fp64:
// thread j adds entries j, j + 256, ... of the span in that order, then the
// block's 256 partials join by the pairwise tree.  fp32 squares are exact in
// fp64, so only the additions round, in an order the blob length fixes.
__global__ __launch_bounds__(256) void sumsq_leaf_kernel(const float* __restrict__ g,
                                                         const unsigned char* __restrict__ mask, long long n,
                                                         double* __restrict__ leaf) {
  __shared__ double r[256];
  const long long base = (long long)blockIdx.x * kNormSpan;
  double acc = 0.0;
  for (int k = 0; k < kNormSpan / 256; ++k) {
    const long long i = base + threadIdx.x + 256 * k;
    if (i < n && mask[i]) {
      const double v = (double)g[i];
      acc = acc + v * v;
    }
  }
  r[threadIdx.x] = acc;
  __syncthreads();
  block_tree_256(r);
  if (threadIdx.x == 0) leaf[blockIdx.x] = r[0];
}

// One segment of a schedule at c = count - boundary, in double, operation by
// operation as the host oracle (zenflow_amd/optim.py) writes it.
__device__ double sched_segment(int kind, const double* __restrict__ p, double c) {
#pragma clang fp contract(off)
  switch (kind) {
    case ZF_SCHED_LINEAR: {
      const double init = p[0], end = p[1], steps = p[2], begin = p[3];
      if (steps <= 0.0) return init;
      const double cc = fmin(fmax(c - begin, 0.0), steps);
      return (init - end) * (1.0 - cc / steps) + end;
    }
    case ZF_SCHED_COSINE: {
      const double init = p[0], steps = p[1], alpha = p[2], ex = p[3];
      const double cc = fmin(c, steps);
      const double d = 0.5 * (1.0 + cos(3.14159265358979323846 * cc / steps));
      return init * ((1.0 - alpha) * pow(d, ex) + alpha);
    }
    case ZF_SCHED_EXPONENTIAL: {
      const double init = p[0], steps = p[1], rate = p[2], begin = p[3];
      const double dc = c - begin;
      if (dc <= 0.0) return init;
      double q = dc / steps;
      if (p[4] != 0.0) q = floor(q);
      double v = init * pow(rate, q);
      if (p[6] != 0.0) v = rate < 1.0 ? fmax(v, p[5]) : fmin(v, p[5]);
      return v;
    }
    case ZF_SCHED_PIECEWISE: {
      double v = p[0];
      const int nb = (int)p[1];
      for (int i = 0; i < nb && i < 3; ++i)
        if (p[2 + 2 * i] < c) v = v * p[3 + 2 * i];
      return v;
    }
    default:
      return p[0];
  }
}

__device__ double sched_value(const zf_schedule& s, double count) {
#pragma clang fp contract(off)
  int k = 0;
  for (int i = 1; i < s.n_segments && i < ZF_SCHED_MAX_SEGMENTS; ++i)
    if (count >= s.boundary[i]) k = i;
  return sched_segment(s.seg_kind[k], s.p[k], k ? count - s.boundary[k] : count);
}

// The step's scalars.  has_clip: norm = sqrt of the leaves' sum (thread j adds
// leaves j, j + 256, ... in that order, then the pairwise tree), clip factor
// max_norm / norm from norm >= max_norm on (optax.clip_by_global_norm), formed
// in double and stored as float; lr(count) likewise; the bias corrections as
// step_update forms them; then count += 1.
__global__ __launch_bounds__(256) void opt_prologue_kernel(OptScalars* __restrict__ sc,
                                                           const double* __restrict__ leaf, int n_leaves,
                                                           int has_clip, float max_norm, int has_lr,
                                                           zf_schedule sched, int has_adam, float b1, float b2) {
#pragma clang fp contract(off)
  __shared__ double r[256];
  double norm = __builtin_nan("");
  if (has_clip) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_leaves; i += 256) acc = acc + leaf[i];
    r[threadIdx.x] = acc;
    __syncthreads();
    block_tree_256(r);
    norm = sqrt(r[0]);
  }
  if (threadIdx.x != 0) return;
  const long long count = sc->count;
  const double t = (double)(count + 1);
  sc->norm = norm;
  sc->clip = has_clip ? (float)(norm < (double)max_norm ? 1.0 : (double)max_norm / norm) : 1.0f;
  sc->lr = has_lr ? (float)sched_value(sched, (double)count) : __builtin_nanf("");
  if (has_adam) {
    sc->bc1 = (float)(1.0 - pow((double)b1, t));
    sc->bc1n = (float)(1.0 - pow((double)b1, t + 1.0));
    sc->bc2 = (float)(1.0 - pow((double)b2, t));
  }
  sc->count = count + 1;
}


// The stages, each on one element in registers (u: the update so far, th:
// the parameter before the step).  The generic loop and the specialised
// forms call the same functions, so a chain has one arithmetic.
__device__ __forceinline__ float stage_adam(float u, float* __restrict__ m, float* __restrict__ v, long long i,
                                            const ChainStage& s, const OptScalars* __restrict__ sc) {
  const float b1 = s.p[0], b2 = s.p[1], eps = s.p[2], eps_root = s.p[3];
  const float mi = b1 * m[i] + (1.0f - b1) * u;
  const float vi = b2 * v[i] + (1.0f - b2) * u * u;
  m[i] = mi;
  v[i] = vi;
  const float mhat = (s.flags & ZF_OPT_FLAG_NESTEROV) ? b1 * (mi / sc->bc1n) + (1.0f - b1) * (u / sc->bc1)
                                                      : mi / sc->bc1;
  const float vhat = vi / sc->bc2;
  return mhat / (sqrtf(vhat + eps_root) + eps);
}

__device__ __forceinline__ float stage_lion(float u, float* __restrict__ mu, long long i, const ChainStage& s) {
  const float b1 = s.p[0], b2 = s.p[1];
  const float mo = mu[i];
  const float c = b1 * mo + (1.0f - b1) * u;
  mu[i] = b2 * mo + (1.0f - b2) * u;
  return c > 0.f ? 1.0f : (c < 0.f ? -1.0f : c);  // jnp.sign: 0 and NaN stay
}

__device__ __forceinline__ float stage_trace(float u, float* __restrict__ tr, long long i, const ChainStage& s) {
  const float decay = s.p[0];
  const float ti = u + decay * tr[i];
  tr[i] = ti;
  return (s.flags & ZF_OPT_FLAG_NESTEROV) ? u + decay * ti : ti;
}

__device__ __forceinline__ float stage_decay(float u, float th, const unsigned char* __restrict__ dmask, long long i,
                                             const ChainStage& s) {
  if ((s.flags & ZF_OPT_FLAG_MASKED) && !dmask[i]) return u;
  return u + s.p[0] * th;
}

__device__ __forceinline__ float stage_clip(float u, const ChainStage& s) {
  return u != u ? u : fminf(fmaxf(u, -s.p[0]), s.p[0]);
}


// theta <- theta + chain(g) on the parameter entries.  The specialised forms
// (what sgd / adam / nadam / adamw / nadamw / lion build) find their stages at
// fixed places after the optional clip: FIRST = CLIP ? 1 : 0, the last stage
// is the learning rate, what lies between is the optional trace / decay.
template <int FORM, bool CLIP>
__global__ void chain_update_kernel(float* __restrict__ prm, const float* __restrict__ g,
                                    const unsigned char* __restrict__ mask,
                                    const unsigned char* __restrict__ dmask, long long n, ChainArgs a,
                                    const OptScalars* __restrict__ sc) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !mask[i]) return;
  const float th = prm[i];
  float u = g[i];
  constexpr int FIRST = CLIP ? 1 : 0;
  if (FORM == kFormGeneric) {
    for (int k = 0; k < a.n; ++k) {
      const ChainStage& s = a.st[k];
      switch (s.kind) {
        case ZF_OPT_CLIP_BY_GLOBAL_NORM: u = u * sc->clip; break;
        case ZF_OPT_CLIP: u = stage_clip(u, s); break;
        case ZF_OPT_SCALE_BY_ADAM: u = stage_adam(u, a.slot[s.slot], a.slot[s.slot + 1], i, s, sc); break;
        case ZF_OPT_SCALE_BY_LION: u = stage_lion(u, a.slot[s.slot], i, s); break;
        case ZF_OPT_TRACE: u = stage_trace(u, a.slot[s.slot], i, s); break;
        case ZF_OPT_ADD_DECAYED_WEIGHTS: u = stage_decay(u, th, dmask, i, s); break;
        case ZF_OPT_SCALE: u = s.p[0] * u; break;
        case ZF_OPT_SCALE_BY_LEARNING_RATE: u = -(sc->lr * u); break;
        default: break;
      }
    }
  } else {
    if (CLIP) u = u * sc->clip;
    if (FORM == kFormSgd) {
      if (a.n == FIRST + 2) u = stage_trace(u, a.slot[0], i, a.st[FIRST]);
    } else {
      if (FORM == kFormAdam) u = stage_adam(u, a.slot[0], a.slot[1], i, a.st[FIRST], sc);
      else u = stage_lion(u, a.slot[0], i, a.st[FIRST]);
      if (a.n == FIRST + 3) u = stage_decay(u, th, dmask, i, a.st[FIRST + 1]);
    }
    u = -(sc->lr * u);
  }
  prm[i] = th + u;
}

}  // namespace

int optim_chain_step(float* prm, const float* g, const unsigned char* mask, const unsigned char* dmask, long long n,
                     const ChainArgs& a, int form, bool clip, float max_norm, bool has_lr, const zf_schedule& sched,
                     bool has_adam, float b1, float b2, OptScalars* sc, double* leaf, int n_leaves, hipStream_t st) {
  if (clip) {
    hipLaunchKernelGGL(sumsq_leaf_kernel, dim3((unsigned)n_leaves), dim3(256), 0, st, g, mask, n, leaf);
    ZF_CHECK_LAUNCH("sumsq_leaf_kernel");
  }
  hipLaunchKernelGGL(opt_prologue_kernel, dim3(1), dim3(256), 0, st, sc, (const double*)leaf, n_leaves, clip ? 1 : 0,
                     max_norm, has_lr ? 1 : 0, sched, has_adam ? 1 : 0, b1, b2);
  ZF_CHECK_LAUNCH("opt_prologue_kernel");
  const unsigned blocks = (unsigned)((n + 255) / 256);
#define ZF_CU(FORM, CLIP)                                                                                 \
  hipLaunchKernelGGL((chain_update_kernel<FORM, CLIP>), dim3(blocks), dim3(256), 0, st, prm, g, mask, dmask, n, a, \
                     (const OptScalars*)sc)
  switch (form) {
    case kFormSgd: if (clip) ZF_CU(kFormSgd, true); else ZF_CU(kFormSgd, false); break;
    case kFormAdam: if (clip) ZF_CU(kFormAdam, true); else ZF_CU(kFormAdam, false); break;
    case kFormLion: if (clip) ZF_CU(kFormLion, true); else ZF_CU(kFormLion, false); break;
    default: ZF_CU(kFormGeneric, false); break;
  }
#undef ZF_CU
  ZF_CHECK_LAUNCH("chain_update_kernel");
  return ZF_OK;
}

int optim_set_count(float* bc, int count, float b1, float b2) {
  hipLaunchKernelGGL(set_count_kernel, dim3(1), dim3(1), 0, nullptr, bc, count, b1, b2);
  ZF_CHECK_LAUNCH("set_count_kernel");
  return ZF_OK;
}

// ---- chain validation (host) ------------------------------------------------
namespace {

// enotsup with a formatted message
int enotsupf(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return enotsup(buf);
}

const char* stage_name(int kind) {
  switch (kind) {
    case ZF_OPT_CLIP_BY_GLOBAL_NORM: return "clip_by_global_norm";
    case ZF_OPT_CLIP: return "clip";
    case ZF_OPT_SCALE_BY_ADAM: return "scale_by_adam";
    case ZF_OPT_SCALE_BY_LION: return "scale_by_lion";
    case ZF_OPT_TRACE: return "trace";
    case ZF_OPT_ADD_DECAYED_WEIGHTS: return "add_decayed_weights";
    case ZF_OPT_SCALE: return "scale";
    case ZF_OPT_SCALE_BY_LEARNING_RATE: return "scale_by_learning_rate";
    default: return nullptr;
  }
}

int stage_slots(int kind) {
  return kind == ZF_OPT_SCALE_BY_ADAM ? 2 : (kind == ZF_OPT_SCALE_BY_LION || kind == ZF_OPT_TRACE) ? 1 : 0;
}

int check_schedule(const zf_schedule& s) {
  if (s.n_segments < 1 || s.n_segments > ZF_SCHED_MAX_SEGMENTS)
    return enotsupf("optimiser chain: a schedule of %d joined segments (at most %d)", s.n_segments,
                   ZF_SCHED_MAX_SEGMENTS);
  for (int k = 0; k < s.n_segments; ++k) {
    if (s.seg_kind[k] < ZF_SCHED_CONSTANT || s.seg_kind[k] > ZF_SCHED_PIECEWISE)
      return einval("optimiser chain: schedule segment %d has unknown kind %d", k, s.seg_kind[k]);
    if (s.seg_kind[k] == ZF_SCHED_PIECEWISE && (s.p[k][1] < 0 || s.p[k][1] > 3))
      return enotsupf("optimiser chain: piecewise_constant_schedule with more than 3 boundaries");
    if (s.seg_kind[k] == ZF_SCHED_COSINE && !(s.p[k][1] > 0))
      return einval("optimiser chain: cosine_decay_schedule needs decay_steps > 0");
    if (s.seg_kind[k] == ZF_SCHED_EXPONENTIAL && !(s.p[k][1] > 0))
      return einval("optimiser chain: exponential_decay needs transition_steps > 0");
  }
  return ZF_OK;
}

}  // namespace

int optim_plan_chain(const zf_optim_chain* chain, bool has_decay_mask, ChainPlan* out) {
  const int S = chain->n_stages;
  if (S < 1) return einval("optimiser chain: no stage");
  if (S > ZF_OPT_MAX_STAGES) return enotsupf("optimiser chain: %d stages (at most %d)", S, ZF_OPT_MAX_STAGES);
  ChainArgs a{};
  a.n = S;
  int slots = 0, n_clip = 0, n_adam = 0, n_lr = 0, lr_at = -1, adam_at = -1;
  bool masked = false;
  for (int k = 0; k < S; ++k) {
    const zf_optim_stage& s = chain->stages[k];
    const char* name = stage_name(s.kind);
    if (!name) return einval("optimiser chain: stage %d has unknown kind %d", k, s.kind);
    if (s.kind == ZF_OPT_CLIP_BY_GLOBAL_NORM) {
      if (++n_clip > 1) return enotsupf("optimiser chain: stage %d: more than one clip_by_global_norm", k);
      if (k != 0)
        return enotsupf("optimiser chain: stage %d: clip_by_global_norm after %s (it must come before every "
                        "stage that changes the update: the norm is the raw gradient's)", k,
                        stage_name(chain->stages[k - 1].kind));
    }
    if (s.kind == ZF_OPT_SCALE_BY_ADAM && ++n_adam > 1)
      return enotsupf("optimiser chain: stage %d: more than one scale_by_adam", k);
    if (s.kind == ZF_OPT_SCALE_BY_LEARNING_RATE) {
      if (++n_lr > 1) return enotsupf("optimiser chain: stage %d: more than one scale_by_learning_rate", k);
      const int rc = check_schedule(s.sched);
      if (rc) return rc;
      lr_at = k;
    }
    if (s.kind == ZF_OPT_SCALE_BY_ADAM) adam_at = k;
    if (s.kind == ZF_OPT_ADD_DECAYED_WEIGHTS && (s.flags & ZF_OPT_FLAG_MASKED)) {
      if (!has_decay_mask)
        return einval("optimiser chain: stage %d: add_decayed_weights is masked but decay_mask is NULL", k);
      masked = true;
    }
    a.st[k].kind = s.kind;
    a.st[k].flags = s.flags;
    a.st[k].slot = slots;
    for (int j = 0; j < 4; ++j) a.st[k].p[j] = s.p[j];
    slots += stage_slots(s.kind);
    if (slots > ZF_OPT_MAX_SLOTS)
      return enotsupf("optimiser chain: stage %d (%s) needs moment array %d (at most %d)", k, name, slots,
                      ZF_OPT_MAX_SLOTS);
  }
  // the forms the aliases build: [clip] body [decay] lr
  const int first = n_clip;
  auto kind = [&](int k) { return k < S ? chain->stages[k].kind : 0; };
  int form = kFormGeneric;
  if (kind(S - 1) == ZF_OPT_SCALE_BY_LEARNING_RATE) {
    if (S == first + 1 || (S == first + 2 && kind(first) == ZF_OPT_TRACE)) form = kFormSgd;
    const bool body_decay = S == first + 3 && kind(first + 1) == ZF_OPT_ADD_DECAYED_WEIGHTS;
    if ((S == first + 2 || body_decay) && kind(first) == ZF_OPT_SCALE_BY_ADAM) form = kFormAdam;
    if ((S == first + 2 || body_decay) && kind(first) == ZF_OPT_SCALE_BY_LION) form = kFormLion;
  }
  ChainPlan p;
  p.args = a;
  p.form = form;
  p.n_slots = slots;
  p.clip = n_clip > 0;
  p.max_norm = n_clip ? chain->stages[0].p[0] : 0.f;
  p.has_lr = lr_at >= 0;
  if (lr_at >= 0) p.sched = chain->stages[lr_at].sched;
  p.has_adam = adam_at >= 0;
  p.b1 = adam_at >= 0 ? chain->stages[adam_at].p[0] : 0.f;
  p.b2 = adam_at >= 0 ? chain->stages[adam_at].p[1] : 0.f;
  p.masked = masked;
  *out = p;
  return ZF_OK;
}

}  // namespace zf
