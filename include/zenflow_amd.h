/*
 * zenflow_amd.h — C ABI of the MI355X-native zenflow hot path (libzenflow_amd.so).
 *
 * The reference (HDembinski/zenflow, a JAX/FLAX library) has no FFI: its
 * boundary is the FLAX module protocol.  Each entry point below replaces one
 * reference callable (cited file:line, relative to the reference repo); the
 * Python package `zenflow_amd` binds them with ctypes and re-exposes the
 * reference's names and signatures (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - Plain pointers and sizes only.  Device pointers come from zf_malloc (or
 *     any hipMalloc'ed buffer); `stream` is a hipStream_t passed as void*
 *     (NULL = the legacy default stream).
 *   - Every function returns 0 on success, a negative ZF_E* code on a bad
 *     argument, or a positive hipError_t.  zf_last_error() returns a
 *     thread-local message for the last failure.
 *   - All floating-point data is fp32, row-major; log-det / NLL partial sums
 *     are fp64.  Kernels never trap on NaN/Inf: they propagate exactly as the
 *     reference does.
 */
#ifndef ZENFLOW_AMD_H
#define ZENFLOW_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZF_OK 0
#define ZF_EINVAL (-1)     /* invalid argument / shape */
#define ZF_ENOTSUP (-2)    /* configuration not supported by the kernels */
#define ZF_ENOMEM (-3)

/* ------------------------------------------------------------------------ */
/* Runtime: devices, memory, streams, events (plumbing for the host layer).  */
/* ------------------------------------------------------------------------ */
const char* zf_last_error(void);
int zf_version(void);
int zf_device_count(int* count);
int zf_set_device(int device);
int zf_get_device(int* device);
int zf_device_name(int device, char* buf, int buflen);
int zf_device_synchronize(void);
int zf_malloc(void** ptr, size_t bytes);
int zf_free(void* ptr);
int zf_memset_async(void* ptr, int value, size_t bytes, void* stream);
/* Host <-> device copies, ordered on `stream`.  htod returns once `src` may be
 * reused (the copy itself completes in stream order); dtoh returns with `dst`
 * filled (up to 4 MiB through a pinned staging buffer). */
int zf_memcpy_htod(void* dst, const void* src, size_t bytes, void* stream);
int zf_memcpy_dtoh(void* dst, const void* src, size_t bytes, void* stream);
int zf_memcpy_dtod(void* dst, const void* src, size_t bytes, void* stream);
int zf_stream_create(void** stream);
int zf_stream_destroy(void* stream);
int zf_stream_synchronize(void* stream);
int zf_event_create(void** event);
int zf_event_destroy(void* event);
int zf_event_record(void* event, void* stream);
int zf_event_elapsed_ms(void* start, void* stop, float* ms);
int zf_event_synchronize(void* event);
/* Work queued on `stream` after this call waits for `event` (hipStreamWaitEvent). */
int zf_stream_wait_event(void* stream, void* event);

/* ------------------------------------------------------------------------ */
/* K1 — spline numerics at the `zenflow.utils` boundary.                     */
/* ------------------------------------------------------------------------ */
/* Replaces utils.rational_quadratic_spline_forward (src/zenflow/utils.py:65-141).
 * x (M,N), dx/dy (M,N,K) normalised widths/heights, slope (M,N,K-1) inner knot
 * derivatives -> y (M,N), log_det (M,) = sum over N of log dy/dx.
 * y and/or log_det may be NULL.
 * Shape limits (both directions): M >= 0, N >= 1, 1 <= K <= 256, else
 * ZF_EINVAL.  One block holds whole rows: K in {4, 8, 16, 32} with 16-byte
 * aligned dx and dy takes N <= 256; every other K or alignment stages its rows
 * through 48 KiB of LDS and needs N <= 256 and N * (3 * ks + 1) <= 12288 with
 * ks = K + 1 (K even) or K + 2 (K odd), i.e. roughly N * (3K + 4) floats —
 * beyond that ZF_ENOTSUP. */
int zf_rqs_forward(const float* x, const float* dx, const float* dy, const float* slope,
                   float* y, float* log_det, int64_t M, int N, int K, void* stream);

/* Replaces utils.rational_quadratic_spline_inverse (src/zenflow/utils.py:144-202). */
int zf_rqs_inverse(const float* y, const float* dx, const float* dy, const float* slope,
                   float* x, int64_t M, int N, int K, void* stream);

/* Replaces utils.squareplus (src/zenflow/utils.py:18-20), elementwise, b = 4 by default. */
int zf_squareplus(const float* x, float* y, int64_t n, float b, void* stream);

/* Replaces utils.softmax_with_threshold (src/zenflow/utils.py:23-34) over rows of K.
 * 1 <= K <= 6144 (one row, at an odd stride, within 48 KiB of LDS), else ZF_EINVAL. */
int zf_softmax_with_threshold(const float* x, float* y, int64_t M, int K, double threshold,
                              void* stream);

/* Replaces utils.normalize_spline_params (src/zenflow/utils.py:37-62):
 * raw (M, K) / (M, K) / (M, K-1) logits -> normalised, written in place.
 * 1 <= K <= 6143 (a dx and a dy row, each at an odd stride, within 48 KiB of
 * LDS), else ZF_EINVAL; slope may be NULL at K = 1. */
int zf_normalize_spline_params(float* dx, float* dy, float* slope, int64_t M, int K,
                               void* stream);

/* ------------------------------------------------------------------------ */
/* Fused flow program: ShiftBounds / NeuralSplineCoupling / Roll / latent.   */
/* ------------------------------------------------------------------------ */

/* Op kinds of a flow program (one per reference bijector). */
#define ZF_OP_SHIFT_BOUNDS 1 /* bijectors.ShiftBounds         bijectors.py:132-273 */
#define ZF_OP_ROLL 2         /* bijectors.Roll                bijectors.py:276-297 */
#define ZF_OP_NSC 3          /* bijectors.NeuralSplineCoupling bijectors.py:300-371 */

/* Latent log_prob epilogues (distributions.py). */
#define ZF_LATENT_NONE 0
#define ZF_LATENT_NORMAL 1    /* distributions.py:50-62  */
#define ZF_LATENT_BETA 2      /* distributions.py:81-116 */
#define ZF_LATENT_TRUNCNORM 3 /* distributions.py:65-78  */
#define ZF_LATENT_UNIFORM 4   /* distributions.py:119-126 */

/* Activation of the conditioner's hidden layers (NSC.act, bijectors.py:319;
 * the flax.linen / jax.nn functions of those names).  Split-MFMA kernel
 * (zf_flow_kernel_variant): all eight on the f16x2 scheme (sigmoid and
 * softplus centred on 1/2 and log 2); under ZF_X3_SCHEME=bf16x3 softplus
 * runs on the fp32 kernel.  The trainer takes all eight. */
#define ZF_ACT_SWISH 0      /* nn.swish = nn.silu: x * sigmoid(x) */
#define ZF_ACT_RELU 1       /* nn.relu */
#define ZF_ACT_TANH 2       /* nn.tanh */
#define ZF_ACT_SIGMOID 3    /* nn.sigmoid */
#define ZF_ACT_GELU 4       /* nn.gelu (approximate=True, the flax default) */
#define ZF_ACT_SOFTPLUS 5   /* nn.softplus = logaddexp(x, 0) */
#define ZF_ACT_ELU 6        /* nn.elu (alpha 1) */
#define ZF_ACT_LEAKY_RELU 7 /* nn.leaky_relu (negative slope 0.01) */
#define ZF_ACT_COUNT 8

/* ShiftBounds per-dim modes (bijectors.py:183-205). */
#define ZF_SB_NONE 0  /* unbounded: running min/max affine + clip        */
#define ZF_SB_BOTH 1  /* (a, b) both finite: fixed affine                */
#define ZF_SB_LOWER 2 /* only a: t = safe_log(x - a), then min/max affine */
#define ZF_SB_UPPER 3 /* only b: t = safe_log(b - x), then min/max affine */

typedef struct zf_op_desc {
  int32_t kind;       /* ZF_OP_* */
  /* ROLL */
  int32_t shift;      /* jnp.roll shift along the last axis */
  /* NSC */
  int32_t knots;      /* K (2 <= K <= 64) */
  int32_t n_hidden;   /* number of hidden Dense layers (len(layers)), 1..16 */
  int32_t hidden[16]; /* widths of the hidden layers (each <= 4096; > 256: the layered path) */
  int32_t act;        /* ZF_ACT_* */
  int32_t _pad;
  /* Offsets (in floats) into the NATURAL parameter blob, filled by
   * zf_flow_plan.  The natural blob holds exactly the FLAX variables:
   *   NSC:  off_bn -> BatchNorm_0 {mean[DC], var[DC], scale[DC], bias[DC]}
   *         (DC = D - D/2 + C conditioner inputs),
   *         off_w[l] -> Dense_l.kernel, row-major (in_l, out_l),
   *         off_b[l] -> Dense_l.bias (out_l); l = 0..n_hidden, the last layer
   *         has out = (D/2)*(3K-1) (bijectors.py:343-347).
   *   SHIFT_BOUNDS: off_sb -> per dim 8 floats {mode(ZF_SB_*), a, b, xmin, xmax, 0, 0, 0}
   *         (batch_stats xmin_i / xmax_i, bijectors.py:243-248). */
  int64_t off_bn;
  int64_t off_w[17];
  int64_t off_b[17];
  int64_t off_sb;
} zf_op_desc;

typedef struct zf_flow_desc {
  int32_t dim;        /* D: data dims (2..64 when the flow has an NSC) */
  int32_t cond_dim;   /* C: condition dims (0 = unconditional) */
  int32_t latent;     /* ZF_LATENT_* */
  float latent_param; /* Beta peakness */
  int32_t n_ops;      /* <= 64 */
  int32_t _pad;
  zf_op_desc ops[64];
} zf_flow_desc;

typedef struct zf_flow zf_flow_t; /* opaque handle: device-resident packed weights */

/* Validate `desc` and fill its natural-blob offsets; *blob_floats = size of
 * the natural blob.  Host-side only. */
int zf_flow_plan(zf_flow_desc* desc, int64_t* blob_floats);

/* Pack the natural blob into the device layout (MFMA fragment order, BN
 * folded to (mean, rsqrt(var+eps)*scale, bias), ShiftBounds mul/log(mul))
 * and copy it to the current device.  The handle owns the device copy until
 * zf_flow_destroy. */
int zf_flow_create(const zf_flow_desc* desc, const float* blob_host, int64_t blob_floats,
                   zf_flow_t** handle);
int zf_flow_destroy(zf_flow_t* handle);

/* Which kernel the handle runs (no reference counterpart: an
 * implementation detail made observable for tests and benchmarks):
 * ZF_KERNEL_FP32 (fp32 MFMA, any shape up to hidden 256), the split-MFMA
 * kernel for the shapes it covers (x3_eligible: every hidden width <= 256,
 * one knot count in 2..32 for all couplings — 8, 16, 32 instantiated, the
 * others padded with inert knots, 31 excepted — dim <= 64) in one of two
 * schemes: ZF_KERNEL_F16X2 (default: two-term fp16 split of
 * power-of-two-scaled operands, three fp16 MFMAs per k-step) or
 * ZF_KERNEL_BF16X3 (three-term bf16 split, six bf16 MFMAs per k-step;
 * ZF_X3_SCHEME=bf16x3, where a softplus coupling runs on the fp32 kernel), or
 * ZF_KERNEL_LAYERED (a hidden width above 256: op by op).  The environment
 * is read at zf_flow_create time; ZF_DISABLE_X3=1 forces ZF_KERNEL_FP32 for
 * fused shapes.  -1 if h is NULL. */
#define ZF_KERNEL_FP32 0
#define ZF_KERNEL_BF16X3 1
#define ZF_KERNEL_F16X2 2
#define ZF_KERNEL_LAYERED 3 /* a hidden width > 256: op by op (BatchNorm, GEMMs, spline kernels) */
int zf_flow_kernel_variant(const zf_flow_t* h);

/* Device workspace needed by zf_flow_log_prob for N rows. */
int64_t zf_flow_workspace_bytes(int64_t N);

/* Replaces Flow.__call__ = log_prob (src/zenflow/flow.py:22-48), eval mode:
 * x (N,D), c (N,C) or NULL -> log_prob (N,) with NaN -> -inf, +-inf -> +-FLT_MAX
 * (jnp.nan_to_num, flow.py:47).  If nll_sum != NULL, the per-block fp64
 * partial sums of log_prob are reduced on device into nll_sum[0]
 * (NLL = -nll_sum/N, train.py:75-78). */
int zf_flow_log_prob(zf_flow_t* h, const float* x, const float* c, float* log_prob,
                     double* nll_sum, void* workspace, int64_t N, void* stream);

/* Segment form of zf_flow_log_prob: runs ops [op_begin, op_end) on x, seeds
 * the log-det accumulator from log_det_in (may be NULL), then applies the
 * latent epilogue (train mode runs the bijectors segment by segment).  With a
 * workspace the kernel writes per-block fp64 partial sums of log_prob there;
 * with nll_sum it also reduces them (else call zf_flow_nll_reduce). */
int zf_flow_log_prob_segment(zf_flow_t* h, int op_begin, int op_end, const float* x,
                             const float* c, const float* log_det_in, float* log_prob,
                             double* nll_sum, void* workspace, int64_t N, void* stream);

/* Fixed-order fp64 sum of the per-block partials a log_prob launch left in
 * `workspace` for N rows -> nll_sum[0] (= sum log_prob; NLL = -nll_sum/N). */
int zf_flow_nll_reduce(const void* workspace, int64_t N, double* nll_sum, void* stream);

/* Launches of the split-MFMA kernels this handle has made, by form: the
 * streaming form, the resident form with its generic frame, the resident form
 * with the frame specialised for D = 4, C = 0, affine ShiftBounds and a Normal
 * latent.  -1 for a NULL handle or an unknown form. */
#define ZF_FORM_STREAMING 0
#define ZF_FORM_RESIDENT 1
#define ZF_FORM_RESIDENT_FRAME 2
int64_t zf_flow_launch_count(const zf_flow_t* h, int form);

/* Replaces Chain.__call__ (bijectors.py:103-111) over the op range
 * [op_begin, op_end): x (N,D) -> y (N,D), log_det (N,).  If log_det_in is not
 * NULL its values seed the accumulator (chained segments, train mode). */
int zf_flow_forward(zf_flow_t* h, int op_begin, int op_end, const float* x, const float* c,
                    float* y, const float* log_det_in, float* log_det, int64_t N,
                    void* stream);

/* Replaces Chain.inverse (bijectors.py:113-116) / the bijector half of
 * Flow.sample (flow.py:70-78) over [op_begin, op_end), applied in reverse:
 * z (N,D) -> x (N,D). */
int zf_flow_inverse(zf_flow_t* h, int op_begin, int op_end, const float* z, const float* c,
                    float* x, int64_t N, void* stream);

/* Replaces Flow.sample (flow.py:50-78) end to end: the latent draw
 * (distributions.py:61-62 / 75-78 / 106-112 / 125-126) happens on the device
 * in the inverse kernel's prologue — Philox4x32-10 keyed by `seed`, counter =
 * (row, dim, stream), so x[row] depends only on (seed, row) — then the whole
 * Chain.inverse runs in the same launch.  c (N,C) or NULL -> x (N,D).
 * jax.random's threefry bits are not reproduced (parity is statistical). */
int zf_flow_sample(zf_flow_t* h, uint64_t seed, const float* c, float* x, int64_t N, void* stream);

/* Replaces Distribution.sample (distributions.py:61-62 Normal, :75-78
 * TruncatedNormal, :106-112 Beta(param, param), :125-126 Uniform): z (N,D)
 * drawn with the same counter-based generator as zf_flow_sample (same seed
 * -> the same z that zf_flow_sample maps through the inverse). */
int zf_latent_sample(int latent, double param, uint64_t seed, float* z, int64_t N, int D, void* stream);

/* Replace one NSC op's BatchNorm statistics (mean[DC], var[DC]) — flax
 * BatchNorm with use_running_average=False normalises by batch statistics. */
int zf_flow_set_bn_stats(zf_flow_t* h, int op, const float* mean, const float* var);

/* Replace one ShiftBounds op's per-dim xmin/xmax (bijectors.py:250-263). */
int zf_flow_set_sb_stats(zf_flow_t* h, int op, const float* xmin, const float* xmax);

/* ------------------------------------------------------------------------ */
/* Train-mode batch statistics (reductions over the batch axis).             */
/* ------------------------------------------------------------------------ */
/* Per column j (0 <= j < ncols) of x (N rows, row stride `ld` floats, first
 * column `col_offset`): min, max (fp32, NaN-propagating like jnp.min/max) and
 * sum, sum of squares (fp64).  ShiftBounds' batch min/max (bijectors.py:250-257)
 * and flax BatchNorm's batch mean/var (bijectors.py:342, train=True).
 * pre_modes/pre_params (host arrays of ncols, or NULL): per column ZF_SB_LOWER
 * -> safe_log(x - a), ZF_SB_UPPER -> safe_log(a - x) with a = pre_params[j]
 * (the one-sided-bound transform, bijectors.py:193-202).  Outputs are device
 * pointers (any may be NULL); workspace: zf_colstats_workspace_bytes(N, ncols). */
int64_t zf_colstats_workspace_bytes(int64_t N, int ncols);
int zf_colstats(const float* x, int64_t N, int ncols, int64_t ld, int col_offset,
                const float* pre_modes, const float* pre_params, float* cmin, float* cmax,
                double* csum, double* csumsq, void* workspace, void* stream);

/* ------------------------------------------------------------------------ */
/* Training — zenflow.train (src/zenflow/train.py:18-138).                    */
/* ------------------------------------------------------------------------ */

/* optax.adamw / optax.nadamw hyper-parameters (train.py:13-16 default:
 * nadamw(learning_rate=1e-3); optax defaults b1 0.9, b2 0.999, eps 1e-8,
 * weight_decay 1e-4). */
typedef struct zf_optim_desc {
  float learning_rate, b1, b2, eps, weight_decay;
  int nesterov; /* 1: nadamw, 0: adamw */
} zf_optim_desc;

typedef struct zf_trainer zf_trainer_t;

/* A trainer owns a device copy of the natural blob (zf_flow_plan layout:
 * parameters AND batch statistics), its gradient and the optimiser moments.
 * param_mask[i] = 1 marks the blob entries that are parameters (updated by
 * the optimiser), 0 the batch statistics.  ShiftBounds rows carry the margin
 * in slot 5.  ShiftBounds is supported as the first op only; conditioner
 * inputs <= 64; batches up to batch_max rows. */
int zf_trainer_create(const zf_flow_desc* desc, const float* blob_host, int64_t blob_floats,
                      const unsigned char* param_mask, int64_t batch_max, const zf_optim_desc* opt,
                      zf_trainer_t** trainer);
int zf_trainer_destroy(zf_trainer_t* trainer);

/* loss_fn of train.py:64-72 and its gradient (jax.grad): train-mode forward
 * (batch statistics) of x (B,D), c (B,C) or NULL on the device; loss[0] (fp64,
 * device) = -mean(log_prob); grad (device, blob layout; NULL: internal) =
 * d loss / d blob (zero on statistics).  update_stats != 0 also applies the
 * running-statistics updates (ShiftBounds min/max, BatchNorm momentum). */
int zf_trainer_loss_grad(zf_trainer_t* trainer, const float* x, const float* c, int64_t B, int update_stats,
                         double* loss, float* grad, void* stream);

/* step of train.py:80-86: loss_grad with statistics update, then the
 * optimiser update of the parameters. */
int zf_trainer_step(zf_trainer_t* trainer, const float* x, const float* c, int64_t B, double* loss,
                    void* stream);

/* Data-parallel training: one trainer per GPU, each
 * on its shard of every global batch.  The trainer exchanges at every batch
 * reduction of loss_fn and its gradient — the ShiftBounds batch min/max
 * (bijectors.py:250-257), the BatchNorm batch sums forward and reverse
 * (bijectors.py:342, flax BatchNorm), the loss (train.py:64-72) and the
 * gradient (train.py:82) — through one primitive:
 *   allgather(ctx, send, recv, bytes, stream): recv[world][bytes] = every
 *   rank's `bytes` of send, in rank order, ordered on `stream`
 * (zf_rccl_allgather with ctx = an RCCL communicator, or any host transport
 * that completes it synchronously).  Every sum is a fixed tree over row
 * leaves whose count depends on the global batch only, and the ranks combine
 * their subtree roots by the top of that tree: every rank gets the same
 * bits, and R ranks (a power of two, equal shards) the bits one device gets
 * on the whole batch.  NULL / world 1: single device (the default). */
typedef int (*zf_allgather_fn)(void* ctx, const void* send, void* recv, size_t bytes, void* stream);
typedef struct zf_comm_desc {
  int rank, world;
  void* ctx;
  zf_allgather_fn allgather;
} zf_comm_desc;
int zf_trainer_set_comm(zf_trainer_t* trainer, const zf_comm_desc* comm);

/* loss_grad / step on this rank's `rows` rows of a global batch of
 * `global_rows` rows (the loss is -mean over the global batch; the gradient
 * and loss returned are the global ones, identical on every rank).  The
 * plain entries above use global_rows = rows * world.  Every loss_grad /
 * step entry checks its arguments first: a call that returns ZF_EINVAL for
 * them has enqueued nothing on the stream. */
int zf_trainer_loss_grad_shard(zf_trainer_t* trainer, const float* x, const float* c, int64_t rows,
                               int64_t global_rows, int update_stats, double* loss, float* grad, void* stream);
int zf_trainer_step_shard(zf_trainer_t* trainer, const float* x, const float* c, int64_t rows, int64_t global_rows,
                          double* loss, void* stream);

/* Gradients with respect to the flow's inputs.  The reference's Flow is a
 * differentiable JAX function (flow.py:22-48) and its users differentiate it
 * with respect to x and c: examples/deep_set.ipynb's DeepSetFlow feeds
 * c = phi(x) into self.flow(y, c, train=train), and jax.grad(loss_fn_2)
 * trains phi together with the flow.
 *
 * Train mode (train.py:64-86): loss_grad / step as above, and gc (device,
 * (rows, C), this rank's rows) = d loss / d c of the GLOBAL loss (scaled by
 * 1 / global_rows), through BatchNorm on batch statistics (the global sums of
 * the reverse pass).  The couplings accumulate in a fixed order: the last
 * coupling assigns, earlier ones add.  gc == NULL or C == 0: exactly the
 * entries above.  loss, grad and the stepped blob have the same bits with
 * and without gc; step with gc launches the kernels eagerly (the captured
 * step graph is the one of zf_trainer_step_shard, unchanged).  d loss / d x
 * in train mode is not provided (ShiftBounds' batch min / max route gradient
 * to the arg-extreme rows). */
int zf_trainer_loss_grad_cond_shard(zf_trainer_t* trainer, const float* x, const float* c, int64_t rows,
                                    int64_t global_rows, int update_stats, double* loss, float* grad,
                                    float* gc, void* stream);
int zf_trainer_step_cond_shard(zf_trainer_t* trainer, const float* x, const float* c, int64_t rows,
                               int64_t global_rows, double* loss, float* gc, void* stream);

/* Weighted maximum likelihood.  With the reference the loss is user-visible
 * JAX, and a user with weighted samples (Monte-Carlo event weights, sWeights,
 * importance weights, class-balance weights) writes
 *   -(w * lp).sum() / w.sum()
 * around flow.apply(..., train=True).  Here: w (device, this rank's `rows`
 * weights, fp32) gives
 *   loss = -sum_b w_b lp_b / Wsum,   Wsum = sum_b w_b over the global batch,
 * lp_b the train-mode log_prob after nan_to_num, as in the entries above.
 *   - The weights enter at the loss only.  BatchNorm's batch mean / variance,
 *     ShiftBounds' batch min / max and the running-statistics updates are taken
 *     over all rows, zero-weight rows included (what the reference computes for
 *     the loss above): the statistics after an update_stats pass have the bits
 *     of the unweighted pass, and a zero-weight row still has a non-zero
 *     d loss / d c through the batch statistics.
 *   - Row b's cotangent is -w_b / Wsum where lp_b is finite before nan_to_num
 *     and 0 elsewhere; Wsum is an fp64 sum over the loss's own leaf tree, so
 *     every rank gets the same bits, and equal power-of-two shards the bits of
 *     one device.  Scaling every weight by a power of two changes no bit.
 *   - Weights may be zero or negative; Wsum must be positive.  That is not
 *     checked here: a non-positive sum gives a non-finite loss.  No index is
 *     derived from a weight.
 *   - loss[0] is the weighted mean as is (fp64).
 * gc as in the _cond_ entries (may be NULL).  w == NULL: exactly the _cond_
 * entries.  The weighted step replays a captured graph of its own per batch
 * size (weighted and unweighted steps may alternate on one trainer); with gc
 * it launches the kernels eagerly. */
int zf_trainer_loss_grad_weighted_shard(zf_trainer_t* trainer, const float* x, const float* c, const float* w,
                                        int64_t rows, int64_t global_rows, int update_stats, double* loss,
                                        float* grad, float* gc, void* stream);
int zf_trainer_step_weighted_shard(zf_trainer_t* trainer, const float* x, const float* c, const float* w,
                                   int64_t rows, int64_t global_rows, double* loss, float* gc, void* stream);

/* Eval mode: the vector-Jacobian product of log_prob (flow.py:22-48 with
 * train=False) at the trainer's current blob — BatchNorm on the stored
 * mean / var, ShiftBounds on the stored xmin / xmax (no batch reductions, no
 * communicator, no statistics update).  x (N,D), c (N,C) or NULL, cot (N,) or
 * NULL (= ones); any of the outputs may be NULL:
 *   log_prob (N,)  with flow.py:47's nan_to_num
 *   gx (N,D)       gx[i] = cot[i] * d log_prob[i] / d x[i]
 *   gc (N,C)       gc[i] = cot[i] * d log_prob[i] / d c[i]
 * Rows whose log_prob is not finite before nan_to_num get all-zero gx and gc
 * rows (the `where` gradient of nan_to_num).  Any N >= 1, processed in chunks
 * of batch_max rows; rows are independent (a row's results depend on its own
 * inputs and on the chunk's row count, which selects the GEMM kernels, only).
 * The trainer's limits apply (ZF_ENOTSUP at zf_trainer_create). */
int zf_trainer_log_prob_vjp(zf_trainer_t* trainer, const float* x, const float* c, const float* cot,
                            float* log_prob, float* gx, float* gc, int64_t N, void* stream);

/* Custom losses.  With the reference the loss is ordinary user code:
 * flow.apply (flow.py:22-48) is a differentiable JAX function and the
 * eighteen lines of train.py:64-86 (loss_fn, jax.grad, the optax update) are
 * what users copy and change — a mixture with an analytic background,
 * importance-weighted or penalised objectives, two flows under one loss,
 * fine-tuning with frozen statistics, accumulated or edited gradients.  Every
 * such loss L(lp_0 .. lp_{B-1}) of the per-row log_prob needs three steps,
 * and these are the three entries:
 *
 * zf_trainer_forward: stages this rank's rows x (rows,D), c (rows,C) or NULL
 *   (rows <= batch_max; global_rows as in the _shard entries) and runs the
 *   forward pass, every activation the reverse pass reads kept in the
 *   trainer.  log_prob (rows,) on the device receives lp with flow.py:47's
 *   nan_to_num.
 *     train != 0  flow.apply(..., train=True): the forward half of
 *                 zf_trainer_loss_grad_shard — batch statistics, exchanged
 *                 over the communicator, and the running-statistics update
 *                 when update_stats != 0 (the same bits as that entry's).
 *     train == 0  flow.apply(..., train=False): the forward of
 *                 zf_trainer_log_prob_vjp (the same log_prob bits) on the
 *                 stored statistics; nothing is exchanged; update_stats must
 *                 be 0 (ZF_EINVAL, nothing enqueued).
 *   The pass stays pending until zf_trainer_backward takes it.  Any of
 *   loss_grad*, step*, log_prob_vjp, set_blob, set_optim_chain,
 *   apply_gradient or another forward drops it.
 *
 * zf_trainer_backward: cot (rows,) fp32 on the device is d L / d lp_b of this
 *   rank's rows (NULL: ones).  grad (blob layout, fp32, device; NULL: the
 *   trainer's own gradient buffer, which the optimiser reads) receives
 *     d / d blob of  sum over the GLOBAL batch of cot_b * nan_to_num(lp_b),
 *   zero on the statistics entries and identical on every rank.  gc (rows,C)
 *   or NULL receives d / d c of the same sum for this rank's rows,
 *   accumulated in the order of the _cond_ entries.
 *     - Rows whose lp is not finite before nan_to_num get cotangent 0 and
 *       contribute exact zeros (the `where` gradient of nan_to_num).
 *     - Eval mode: rows with cot == 0 contribute exact zeros.  Train mode:
 *       they still enter through the batch statistics, as zero-weight rows of
 *       the weighted loss do.
 *     - Train mode is the reverse half of the weighted loss_grad with cot in
 *       place of -w_b / Wsum: BatchNorm's reverse with its global sums, the
 *       fp64 gradient shares gathered over the ranks.  Eval mode reverses
 *       BatchNorm through the stored statistics (no batch term), forms the
 *       scale / bias gradients from the column sums of gUbn * Uhat and gUbn
 *       over the same leaf tree, and exchanges only the final gradient.
 *   Needs a pending forward (ZF_EINVAL "no forward pending", nothing
 *   enqueued); one backward per forward.
 *
 * zf_trainer_apply_gradient: the optimiser half of a step on grad (device,
 *   blob layout; NULL: the trainer's own buffer) — the (n)adamw update or the
 *   chain of zf_trainer_set_optim_chain; the step counter, the schedule and
 *   the moments advance as in zf_trainer_step.  It does not communicate:
 *   every rank passes the same gradient, which is what backward returns.
 *
 * All three launch eagerly on `stream`; the captured step graphs are the
 * zf_trainer_step* entries' alone. */
int zf_trainer_forward(zf_trainer_t* trainer, const float* x, const float* c, int64_t rows, int64_t global_rows,
                       int train, int update_stats, float* log_prob, void* stream);
int zf_trainer_backward(zf_trainer_t* trainer, const float* cot, float* grad, float* gc, void* stream);
int zf_trainer_apply_gradient(zf_trainer_t* trainer, const float* grad, void* stream);

/* Gradients through sampling.  With the reference
 * x = flow.apply(vars, c_or_n, method="sample") (flow.py:50-78) is an
 * ordinary JAX function, and jax.grad of any loss of the samples works: the
 * reverse-KL / variational fit E_z[log q(x(z)) - log p(x(z))] to a target
 * density, amortised posteriors q(theta | c), importance-sampling proposals,
 * samples fed to a differentiable simulator or a discriminator.  Two entries,
 * with zf_trainer_apply_gradient as the optimiser half:
 *
 * zf_trainer_sample_forward: z (rows,D) latent rows and c (rows,C) or NULL on
 *   the device (rows <= batch_max; rows / global_rows as zf_trainer_forward's
 *   in eval mode, except that one device may pass global_rows > rows for a
 *   micro-batch of a larger batch: rows are independent, global_rows only
 *   picks the GEMM forms and the reduction leaves; nothing is exchanged).
 *   x (rows,D) receives
 *   bijector.inverse(z, c) as Flow.sample computes it (flow.py:76-77): eval
 *   mode, BatchNorm on the stored mean / var (bijectors.py:367-371),
 *   ShiftBounds.inverse on the stored xmin / xmax (:210-240), Roll.inverse.
 *   log_q (rows,) or NULL receives
 *     latent.log_prob(z) + sum over the ops of log_det_op,
 *   log_det_op the op's FORWARD log-det (utils.py:121-139,
 *   bijectors.py:186-207) at the inverse's own intermediate for that op:
 *   what flow.apply(vars, x, c) gives for the sample before nan_to_num, up to
 *   float32 rounding, wherever ShiftBounds' clamp is inactive.  A log_q that
 *   is not finite is reported as such (-inf / +inf where the latent density
 *   is, NaN from a NaN log-det), not as finfo.min.
 *   A row whose spline inverse is not finite (the idx == K sliver of the
 *   reference's fill-mode gather, utils.py:224-230) comes out as NaN in every
 *   column of x, where the reference has NaN in the columns that depend on it.
 *   ZF_EINVAL (nothing enqueued) while a ShiftBounds dim's stored bounds are
 *   still the initial +-inf.  The pass stays pending for one
 *   zf_trainer_sample_backward; the calls that drop a pending
 *   zf_trainer_forward drop it too.  zf_trainer_backward does not take it
 *   (ZF_EINVAL "no forward pending", nothing enqueued).
 *
 * zf_trainer_sample_backward: gx (rows,D) = d L / d x and glq (rows,) =
 *   d L / d log_q of this rank's rows (glq NULL: zeros), on the device.  grad
 *   (blob layout, fp32, device; NULL: the trainer's own buffer) receives
 *     d / d blob of  sum over the GLOBAL batch of gx_b . x_b + glq_b log_q_b,
 *   zero on the statistics entries and identical on every rank (only this
 *   final gradient is exchanged); gz (rows,D) or NULL the same sum's gradient
 *   with respect to z, gc (rows,C) or NULL with respect to c.
 *     - The x path is the derivative of the reference's own inverse formula,
 *       the quadratic root of utils.py:193-201 with the bin found on the yk
 *       knots: no clamp, no epsilons.  (Not 1 / s'(x) of the forward spline,
 *       whose den + 1e-5 and clamp make its derivative differ by ~1e-5.)
 *     - The log_q path is the forward spline's reverse at x_t with the row's
 *       glq as the log-det cotangent; its d / d x_t joins the cotangent on x_t
 *       before the root formula is reversed.
 *     - Latent columns outside [0, 1) are the identity: the cotangent passes
 *       through and no parameter gradient arises.
 *     - Rows whose x or log_q is not finite (the sliver above; a latent value
 *       outside the latent's support) contribute exact zeros to grad and get
 *       all-zero gz / gc rows: zf_trainer_backward's rule.  A deliberate
 *       deviation: jax.grad would make the whole gradient NaN.
 *   Needs a pending zf_trainer_sample_forward (ZF_EINVAL "no forward pending",
 *   nothing enqueued: a pending zf_trainer_forward does not count); one
 *   backward per forward.
 * The trainer's limits apply (ZF_ENOTSUP at zf_trainer_create). */
int zf_trainer_sample_forward(zf_trainer_t* trainer, const float* z, const float* c, int64_t rows,
                              int64_t global_rows, float* x, float* log_q, void* stream);
int zf_trainer_sample_backward(zf_trainer_t* trainer, const float* gx, const float* glq, float* grad, float* gz,
                               float* gc, void* stream);

/* Copy the trainer's natural blob (parameters + statistics) out / in. */
int zf_trainer_get_blob(zf_trainer_t* trainer, float* blob_host);
int zf_trainer_set_blob(zf_trainer_t* trainer, const float* blob_host);

/* ------------------------------------------------------------------------ */
/* Optimiser chains — optax.GradientTransformation, which the reference's    */
/* train() takes (train.py:27, 62, 84-85), restated from optax's published   */
/* formulas (optax is not a dependency).  count = updates already applied,   */
/* t = count + 1; u starts as the gradient, the step ends with theta += u.   */
/* ------------------------------------------------------------------------ */

/* Stage kinds; p[] and flags of zf_optim_stage per kind. */
#define ZF_OPT_CLIP_BY_GLOBAL_NORM 1   /* optax.clip_by_global_norm: p[0] max_norm */
#define ZF_OPT_CLIP 2                  /* optax.clip: p[0] max_delta */
#define ZF_OPT_SCALE_BY_ADAM 3         /* optax.scale_by_adam: p = b1, b2, eps, eps_root; NESTEROV */
#define ZF_OPT_SCALE_BY_LION 4         /* optax.scale_by_lion: p = b1, b2 */
#define ZF_OPT_TRACE 5                 /* optax.trace: p[0] decay; NESTEROV */
#define ZF_OPT_ADD_DECAYED_WEIGHTS 6   /* optax.add_decayed_weights: p[0] weight_decay; MASKED */
#define ZF_OPT_SCALE 7                 /* optax.scale: p[0] step_size */
#define ZF_OPT_SCALE_BY_LEARNING_RATE 8 /* optax.scale_by_learning_rate: u <- -lr(count) u; sched */
#define ZF_OPT_FLAG_NESTEROV 1
#define ZF_OPT_FLAG_MASKED 2           /* add_decayed_weights only where decay_mask is set */
#define ZF_OPT_MAX_STAGES 8
#define ZF_OPT_MAX_SLOTS 4             /* moment arrays: adam 2 (m, v), lion 1, trace 1 */

/* Schedule kinds (optax.schedules); p[] of a segment per kind. */
#define ZF_SCHED_CONSTANT 0     /* optax.constant_schedule: p[0] value */
#define ZF_SCHED_LINEAR 1       /* optax.linear_schedule: p = init, end, transition_steps, transition_begin */
#define ZF_SCHED_COSINE 2       /* optax.cosine_decay_schedule: p = init, decay_steps, alpha, exponent */
#define ZF_SCHED_EXPONENTIAL 3  /* optax.exponential_decay: p = init, transition_steps, decay_rate,
                                   transition_begin, staircase (0 / 1), end_value, has_end_value (0 / 1) */
#define ZF_SCHED_PIECEWISE 4    /* optax.piecewise_constant_schedule: p = init, n, b0, s0, b1, s1, b2, s2:
                                   init times every scale s_i whose boundary b_i < count */
#define ZF_SCHED_JOIN 5         /* optax.join_schedules: the top-level kind of n_segments > 1 */
#define ZF_SCHED_MAX_SEGMENTS 4
#define ZF_SCHED_PARAMS 8

/* A schedule count -> value, evaluated on the device in double from the
 * device's own step counter.  n_segments == 1: seg_kind[0] (== kind) on
 * p[0].  optax.join_schedules: kind ZF_SCHED_JOIN, segment k (the last one
 * with count >= boundary[k]; boundary[0] = 0) sees count - boundary[k]. */
typedef struct zf_schedule {
  int kind;
  int n_segments;
  int seg_kind[ZF_SCHED_MAX_SEGMENTS];
  double boundary[ZF_SCHED_MAX_SEGMENTS];
  double p[ZF_SCHED_MAX_SEGMENTS][ZF_SCHED_PARAMS];
} zf_schedule;

typedef struct zf_optim_stage {
  int kind;   /* ZF_OPT_* */
  int flags;  /* ZF_OPT_FLAG_* */
  float p[4];
  zf_schedule sched; /* ZF_OPT_SCALE_BY_LEARNING_RATE only */
} zf_optim_stage;

/* optax.chain: the stages in order. */
typedef struct zf_optim_chain {
  int n_stages; /* 1 .. ZF_OPT_MAX_STAGES */
  int _pad;
  zf_optim_stage stages[ZF_OPT_MAX_STAGES];
} zf_optim_chain;

/* Replace the trainer's optimiser (zf_optim_desc's (n)adamw) by a chain;
 * zf_trainer_step* then run it on the device, inside the captured step graph
 * too.  decay_mask: one byte per blob entry (optax's `mask` of
 * add_decayed_weights, lowered to the blob) or NULL (every parameter).
 * Synchronises, drops the cached step graphs, allocates one zeroed blob-sized
 * array per moment and resets the count.  ZF_ENOTSUP (the message names the
 * stage): more than ZF_OPT_MAX_STAGES stages or ZF_OPT_MAX_SLOTS moment
 * arrays, more than one clip_by_global_norm, or one that follows a stage
 * that changes u (the norm is that of the raw gradient). */
int zf_trainer_set_optim_chain(zf_trainer_t* trainer, const zf_optim_chain* chain,
                               const unsigned char* decay_mask);

/* optax's optimiser state, for checkpoints: moment array `slot` (blob
 * layout, blob_floats host floats) in chain order — scale_by_adam: mu, nu;
 * scale_by_lion: mu; trace: trace.  Without a chain: 0 = m, 1 = v of the
 * (n)adamw update. */
int zf_trainer_get_opt_slot(zf_trainer_t* trainer, int slot, float* host_floats);
int zf_trainer_set_opt_slot(zf_trainer_t* trainer, int slot, const float* host_floats);

/* count (optax's ScaleByAdamState.count and its like), and what the last
 * step used: the learning rate and the gradient's global norm (NaN without
 * clip_by_global_norm).  Any pointer may be NULL.  set_opt_count restores the
 * counter (and the bias corrections that follow from it). */
int zf_trainer_get_opt_scalars(zf_trainer_t* trainer, int64_t* count, double* learning_rate, double* grad_norm);
int zf_trainer_set_opt_count(zf_trainer_t* trainer, int64_t count);

/* ------------------------------------------------------------------------ */
/* Conditioning networks — the `Phi` of examples/deep_set.ipynb: the network  */
/* that produces the flow's condition and is trained together with the flow   */
/* (cells `class NNBlock` / `class Phi` / `class DeepSetFlow` / `loss_fn_2`): */
/*   BatchNorm -> (Dense, act) x depth -> Dense -> Dropout -> sum over sets   */
/* The FLAX layers are restated (flax.linen.BatchNorm / Dense / Dropout, as   */
/* the couplings' are), not called: no JAX is at hand.                        */
/* ------------------------------------------------------------------------ */

/* Segment sum over ragged sets — replaces `sum_matrix @ x` of Phi.__call__
 * (the BCOO matrix that `preprocess` builds has one 1 per element row, in the
 * row of its set; `off` is its CSR form: set s owns rows [off[s], off[s+1])).
 *
 *   out[s, f] = sum over i in [off[s], off[s+1]) of d(i, f),  0 <= f < F <= 64
 *   d(i, f)   = h[i, f]                                  (rate == 0)
 *             = keep(i, f) ? h[i, f] / (1 - rate) : 0    (0 < rate < 1, below)
 *
 * Offsets: S + 1 int64 on the device.  Before use they are clamped,
 *   o[s] = max over j <= s of min(max(off[j], 0), rows),
 * so any content of `off` addresses rows inside h only; host callers
 * validate instead (zenflow_amd.nn).  Rows covered by no set are ignored;
 * an empty set gives a row of +0.
 *
 * Order of the additions (fp32, no atomics).  It depends on the set's length
 * n and on F alone — not on S, the grid, the set's place in the batch or its
 * neighbours — so a set has the same bits wherever it stands:
 *   - the set's rows are cut, from its first row, into chunks of
 *     ZF_SEG_CHUNK rows (the last one shorter); one wave sums one chunk;
 *   - with R = 64 / F (integer division) rows of a chunk per wave step, lane
 *     (j, f), j < R, adds rows j, j + R, j + 2R, ... of the chunk in that
 *     order, starting from +0;
 *   - the chunk's sum of column f is ((p_0 + p_1) + p_2) + ... over the lane
 *     partials p_j, j = 0 .. R - 1;
 *   - the set's chunk sums, in chunk order, are a list of rows again and are
 *     summed by the same three rules, level after level, until one is left.
 * Long sets are thereby spread over many waves at every level: a batch with
 * one set of 10^5 rows among sets of tens does not run as long as its longest
 * set.
 *
 * set_index (rows int32, or NULL): receives set(i), the set that owns row i,
 * or -1 for a row in no set — what zf_segment_bcast reads.
 * workspace: zf_segment_workspace_bytes(rows, S, F) bytes on the device.
 * ZF_EINVAL: NULL h / off / out / workspace, rows < 0, S < 0, F < 1, rate
 * outside [0, 1); ZF_ENOTSUP: F > 64, S > 2^24, rows > 2^31 - 1.  Nothing is
 * enqueued then. */
#define ZF_SEG_CHUNK 512
int64_t zf_segment_workspace_bytes(int64_t rows, int64_t sets, int F);
int zf_segment_sum(const float* h, int64_t rows, int F, const int64_t* off, int64_t sets, float rate,
                   uint64_t seed, float* out, int32_t* set_index, void* workspace, void* stream);

/* Its reverse — the gradient of `sum_matrix @ Dropout(x)` with respect to x:
 *   g_h[i, f] = gc[set(i), f] * keep(i, f) / (1 - rate),
 * and 0 for rows in no set (set_index[i] outside [0, S): never dereferenced).
 * rate == 0: a plain gather of gc rows.  Same error codes. */
int zf_segment_bcast(const float* gc, const int32_t* set_index, int64_t rows, int F, int64_t sets, float rate,
                     uint64_t seed, float* g_h, void* stream);

/* Mean and max over ragged sets — replace `jnp.mean(x, axis=...)` /
 * `jnp.max(x, axis=...)` over a set's rows in Phi.__call__, where a user of
 * the reference edits the pooling line (deep sets' three standard
 * reductions; the max is PointNet's).  pool: ZF_POOL_SUM | ZF_POOL_MEAN |
 * ZF_POOL_MAX; d(i, f), the clamped offsets o, n_s = o[s+1] - o[s], rows in no
 * set and the other arguments as zf_segment_sum's.
 *   SUM   zf_segment_sum itself: the same launches, the same bits.
 *   MEAN  out[s, f] = sum_s[f] / (float)n_s, sum_s the bits zf_segment_sum
 *         returns, one IEEE fp32 division; an empty set gives a row of +0.
 *   MAX   out[s, f] = max over the set's rows of d(i, f).  A NaN anywhere in
 *         the (set, column) gives NaN (as jnp.max; fmaxf alone would drop
 *         it); +-inf are values; an empty set gives a row of +0.  The maximum
 *         is exact: only the sign of a zero depends on the order.  Dropped
 *         entries are zeros that take part (Dropout, then the pooling).  The
 *         levels are the sum's: one wave per ZF_SEG_CHUNK rows, until every
 *         set is down to one chunk.
 * count (sets x F int32, or NULL): MEAN n_s in every column; MAX t[s, f], the
 * number of the set's rows with d(i, f) == out[s, f] (for a NaN maximum the
 * NaN entries), counted in int32 over one more pass over h; SUM untouched.
 * workspace: zf_segment_pool_workspace_bytes(rows, sets, F, pool) bytes (0
 * for arguments the entry rejects).  No atomics: the same bits every call.
 * Limits and error codes are zf_segment_sum's; ZF_EINVAL also for an unknown
 * pool.  Nothing is enqueued then. */
#define ZF_POOL_MEAN 2
#define ZF_POOL_MAX 3
int64_t zf_segment_pool_workspace_bytes(int64_t rows, int64_t sets, int F, int pool);
int zf_segment_pool(const float* h, int64_t rows, int F, const int64_t* off, int64_t sets, int pool, float rate,
                    uint64_t seed, float* out, int32_t* set_index, int32_t* count, void* workspace, void* stream);

/* Their reverse — the gradient of `jnp.mean` / `jnp.max` over the sets of
 * Dropout(x) with respect to x:
 *   MEAN  g_d[i, f] = gc[set(i), f] / (float)n_set(i)
 *   MAX   g_d[i, f] = d(i, f) == out[s, f] ? gc[s, f] / (float)t[s, f] : 0,
 *         s = set(i): the gradient is split evenly among ties, the convention
 *         of jnp.max's gradient and of torch.scatter_reduce(reduce="amax");
 *         for a NaN maximum the NaN entries are the ties.  With dropout every
 *         dropped entry of a column whose kept values are all negative ties
 *         at 0.
 *   g_h[i, f] = g_d[i, f] * keep(i, f) / (1 - rate), and 0 for rows in no set
 *   (or whose count is 0), exactly as zf_segment_bcast applies it.
 * h and out (the forward's input and result) are read for MAX only, count
 * (the forward's) for MEAN and MAX; SUM is zf_segment_bcast itself.  ZF_EINVAL
 * for an unknown pool and for a NULL pointer the mode reads; otherwise
 * zf_segment_bcast's codes. */
int zf_segment_pool_bcast(const float* gc, const int32_t* set_index, int64_t rows, int F, int64_t sets, int pool,
                          float rate, uint64_t seed, const float* h, const float* out, const int32_t* count,
                          float* g_h, void* stream);

/* Repeat over ragged sets — replaces `jnp.repeat(c, sizes, axis=0)` of
 * DeepSetFlow.sample, with the sizes in CSR form (off[s + 1] - off[s] copies
 * of row s):
 *   out[i, :] = c[set(i), :]  for every row i < rows,  0 < F <= 64,
 * and +0 for a row in no set (before the first offset, from the last one on,
 * padding).  c: (sets, F) on the device; off: sets + 1 int64 on the device,
 * clamped before use by the rule of zf_segment_sum, so any content of `off`
 * reads inside c and writes inside out only; out: (rows, F).
 * set_index (rows int32, or NULL) receives set(i) or -1, exactly as
 * zf_segment_sum writes it.  workspace: zf_segment_workspace_bytes(rows,
 * sets, F) bytes.  One search over the clamped offsets per row: the time does
 * not depend on how the rows are divided into sets.  No atomics: a copy, the
 * same bits every time.  Its reverse (the gradient with respect to c) is
 * zf_segment_sum of the rows' gradients with rate 0 over the same offsets.
 * Limits and error codes are zf_segment_sum's (there is no rate), returned
 * before anything is enqueued. */
int zf_segment_repeat(const float* c, int64_t sets, int F, const int64_t* off, int64_t rows, float* out,
                      int32_t* set_index, void* workspace, void* stream);

/* Take whole sets by index — a minibatch of ragged sets packed on the device,
 * what `x[np.concatenate([np.arange(off[s], off[s + 1]) for s in take])]` and
 * a cumsum of the taken lengths do on the host (the element rows of B of S
 * sets drawn at random, contiguous, with their CSR offsets rebuilt):
 *   len_t          = o[take[t] + 1] - o[take[t]],  0 for take[t] outside [0, sets)
 *   off_out[0]     = 0
 *   off_out[t + 1] = min(off_out[t] + len_t, rows_out),         0 <= t < take_n
 *   out[off_out[t] + j, :] = x[o[take[t]] + j, :],  j < off_out[t + 1] - off_out[t]
 * in the set's own order, and +0 in the rows from off_out[take_n] to rows_out
 * (rows_out below the sum of the lengths truncates: the last sets come out
 * shortened or empty).  x: (rows, F) on the device, 0 < F <= 64; off: sets + 1
 * int64 on the device, o its clamped form by the rule of zf_segment_sum, so
 * any content of `off` reads inside x only; take: take_n int64 on the device,
 * not validated but made harmless (an index outside [0, sets) is an empty
 * set), duplicates allowed (bootstrap resampling); out: (rows_out, F);
 * off_out: take_n + 1 int64.  Nothing at or beyond out + rows_out * F is
 * written.
 * off == NULL (unit mode): every set is one row, o[s] = s, sets == rows — the
 * row gather out[t] = x[take[t]] (the per-set targets of a minibatch).
 * workspace: zf_segment_take_workspace_bytes(sets, take_n) bytes on the
 * device (0 for arguments the entry rejects).  One search over off_out per
 * output row: the time does not depend on how the rows are divided into sets.
 * No atomics: a copy, the same bits every time.  Nothing synchronises with
 * the host; take_n == 0 or rows_out == 0 enqueue memsets only.
 * ZF_EINVAL: NULL x / take / out / off_out / workspace, a negative count, F
 * outside 1 .. 64, off == NULL with sets != rows; ZF_ENOTSUP: sets or take_n >
 * 2^24, rows or rows_out > 2^31 - 1.  Nothing is enqueued then. */
int64_t zf_segment_take_workspace_bytes(int64_t sets, int64_t take_n);
int zf_segment_take(const float* x, int64_t rows, int F, const int64_t* off, int64_t sets, const int64_t* take,
                    int64_t take_n, int64_t rows_out, float* out, int64_t* off_out, void* workspace, void* stream);

/* Dropout — replaces nn.Dropout(rate, deterministic=not train) of Phi.__call__:
 *   keep(i, f) = u01_co(philox_at(seed, i, f, ZF_DROPOUT_STREAM).v[ZF_DROPOUT_WORD]) >= rate
 * with i the element row, f the column, Philox4x32-10 and u01_co (top 24
 * bits / 2^24) as in zf_flow_sample; kept entries are divided by
 * (float)1 - rate.  The mask is a function of (seed, i, f): the reverse pass
 * recomputes it.  rate == 0 draws nothing.  jax.random's bits (the
 * `rngs={"dropout": key}` stream) are not reproduced: parity is statistical. */
#define ZF_DROPOUT_STREAM 0x64726f70u /* "drop" */
#define ZF_DROPOUT_WORD 0

#define ZF_POOL_NONE 0 /* one output row per input row (an NNBlock behind BatchNorm) */
#define ZF_POOL_SUM 1  /* Phi: one output row per set */
/* ZF_POOL_MAX (3): one output row per set, zf_segment_pool's max.  ZF_POOL_MEAN (2) is a mode of
 * zf_segment_pool alone: zf_condnet_plan rejects it, as it rejects every other code. */

/* Replaces the configuration of Phi / NNBlock (out_dim, depth, width, act):
 *   BatchNorm(use_running_average=not train)         when batch_norm
 *   Dense(hidden[l]) + act, l = 0 .. n_hidden - 1
 *   Dense(out_dim)
 *   Dropout(dropout, deterministic=not train)
 *   sum / max over each set's rows                    when pool == ZF_POOL_SUM / ZF_POOL_MAX
 * Limits: 1 <= in_dim <= 64, 0 <= n_hidden <= 16, 1 <= hidden[l] <= 4096,
 * 1 <= out_dim <= 64, 0 <= dropout < 1 (ZF_ENOTSUP beyond the sizes,
 * ZF_EINVAL for the rest).  The offsets (in floats) into the natural blob are
 * filled by zf_condnet_plan; every tensor starts at a multiple of 4 floats:
 *   off_bn   -> BatchNorm_0 {mean[in_dim], var[in_dim], scale[in_dim], bias[in_dim]}
 *               (-1 without batch_norm)
 *   off_w[l] -> Dense_l.kernel, row-major (in_l, out_l); off_b[l] -> Dense_l.bias;
 *               l = 0 .. n_hidden, the last layer has out = out_dim. */
typedef struct zf_condnet_desc {
  int32_t in_dim;
  int32_t n_hidden;
  int32_t hidden[16];
  int32_t out_dim;
  int32_t act;        /* ZF_ACT_* */
  int32_t batch_norm; /* 0 / 1 */
  int32_t pool;       /* ZF_POOL_* */
  float dropout;
  int32_t _pad;
  int64_t off_bn;
  int64_t off_w[17];
  int64_t off_b[17];
} zf_condnet_desc;

typedef struct zf_condnet zf_condnet_t;

/* Validate `desc` and fill its offsets; *blob_floats = size of the natural
 * blob (padding between tensors included).  Host-side only. */
int zf_condnet_plan(zf_condnet_desc* desc, int64_t* blob_floats);

/* A handle owns a device copy of the blob (parameters and BatchNorm
 * statistics), the activations of one pass of up to rows_max element rows in
 * up to sets_max sets, the gradient and the optimiser state.  param_mask as
 * zf_trainer_create's (1: parameter, 0: statistics or padding).  optim: the
 * (n)adamw of zf_optim_desc, run as the chain scale_by_adam ->
 * add_decayed_weights -> scale_by_learning_rate (NULL: optax.nadamw(1e-3),
 * train.py:13-16).  What only a train-mode pass, its reverse and the
 * optimiser read (pre-activations, gradients, the 128 MB split-K workspace) is
 * allocated by the first call that needs it: a handle that only evaluates
 * holds the blob and one activation per layer. */
int zf_condnet_create(const zf_condnet_desc* desc, const float* blob_host, int64_t blob_floats,
                      const unsigned char* param_mask, int64_t rows_max, int64_t sets_max,
                      const zf_optim_desc* optim, zf_condnet_t** handle);
int zf_condnet_destroy(zf_condnet_t* handle);

/* Replaces Phi.__call__(x, sum_matrix, train) (and deep_set_flow.apply(...,
 * train=True, mutable=["batch_stats"], rngs={"dropout": key}) for its phi
 * half): x (rows, in_dim) on the device -> c_out, (sets, out_dim) with
 * ZF_POOL_SUM / ZF_POOL_MAX (off: sets + 1 offsets on the device, as zf_segment_sum's) or
 * (rows, out_dim) with ZF_POOL_NONE (off must be NULL; sets is ignored).
 *   train != 0  BatchNorm on the statistics of all `rows` rows passed (padding
 *               rows included: what nn.BatchNorm sees in the example), biased
 *               variance, eps 1e-5, the rule of the couplings' BatchNorm
 *               (bn_stats_kernel); update_stats != 0 also moves the running
 *               statistics (0.99 old + 0.01 batch).  Dropout with `seed`.
 *               Every activation the reverse pass reads is kept; the pass
 *               stays pending for one zf_condnet_backward.
 *   train == 0  the stored statistics, no dropout (`seed` is ignored);
 *               update_stats must be 0; nothing stays pending.
 * ZF_EINVAL (nothing enqueued): NULL x / c_out, rows outside [1, rows_max],
 * sets outside [1, sets_max] or a NULL off with a pooled network, a non-NULL off
 * with ZF_POOL_NONE, update_stats without train.  Every call drops a pending
 * pass first. */
int zf_condnet_forward(zf_condnet_t* handle, const float* x, int64_t rows, const int64_t* off, int64_t sets,
                       int train, int update_stats, uint64_t seed, float* c_out, void* stream);

/* Data-parallel conditioning networks: one handle per GPU, each holding
 * whole sets of every global pass (a set lives on one rank).  The rules are
 * zf_trainer_set_comm's: NULL / world 1 is a single device (the default),
 * ZF_EINVAL for a bad rank or world and for a world above 1 without
 * allgather, ZF_ENOTSUP above 64 ranks; the handle allocates the gather
 * buffer, world x max(blob floats, 256) doubles.  A pending pass is dropped.
 * Under a communicator at most three all-gathers of the ranks' fp64 subtree
 * roots run per step, each combined by the top of the leaf tree
 * (zf_reduce.h): BatchNorm's batch sums in a train-mode forward, its reverse
 * sums in zf_condnet_backward_input (a network with BatchNorm only), and the
 * gradient at the end of either reverse entry — one for a network without
 * BatchNorm.  Sum and max pooling, the tie counts and dropout are per set or
 * per element: nothing is exchanged for them.  Every rank gets the same
 * gradient, statistics and (after zf_condnet_apply_gradient) parameters and
 * optimiser state, bit for bit, for any split of whole sets; R ranks, R a
 * power of two, with global_rows / R element rows each and global_rows a
 * multiple of the leaf count, get the bits one device gets on the
 * concatenated batch. */
int zf_condnet_set_comm(zf_condnet_t* handle, const zf_comm_desc* comm);

/* zf_condnet_forward on this rank's `rows` element rows of a global pass of
 * global_rows rows, of which this rank's first is global row row_base: x,
 * off (offsets local to x) and sets are this rank's own, c_out is (sets,
 * out_dim) for this rank's sets ((rows, out_dim) with ZF_POOL_NONE).  The
 * BatchNorm statistics are those of all global_rows rows, the dropout mask is
 * keep(row_base + i, f), and global_rows picks the GEMM forms and the leaf
 * layouts, so a shard runs the tile form of the one-device pass.
 * zf_condnet_forward is the view with global_rows = rows, row_base = 0.
 * The reverse entries read global_rows and row_base from the pending pass;
 * their grad_out and the kept gradient are the global gradient, identical on
 * every rank, while gc and gx_out hold this rank's rows.  Every rank must
 * make the same calls in the same order.  ZF_EINVAL with nothing enqueued, on
 * top of zf_condnet_forward's: global_rows < rows, row_base < 0, row_base +
 * rows > global_rows, or world 1 and global_rows != rows. */
int zf_condnet_forward_shard(zf_condnet_t* handle, const float* x, int64_t rows, int64_t global_rows,
                             int64_t row_base, const int64_t* off, int64_t sets, int train, int update_stats,
                             uint64_t seed, float* c_out, void* stream);

/* Replaces jax.grad(loss_fn_2) for phi's parameters: gc (device, the shape of
 * the pending forward's c_out) = d loss / d c, e.g. the gc of
 * zf_trainer_step_cond_shard, of zf_trainer_sample_backward or of
 * zf_trainer_log_prob_vjp.  grad_out (blob layout, fp32, device; may be NULL)
 * receives d loss / d blob, zero on statistics and padding; the handle keeps
 * a copy for zf_condnet_apply_gradient.  Weight and bias gradients are the
 * trainer's fixed-order leaf trees (zf_reduce.h) over the element rows.
 * d / d x is not formed here (zf_condnet_backward_input forms it).  One
 * reverse per train-mode forward, through either entry: ZF_EINVAL "no
 * forward pending" (nothing enqueued) otherwise — after an eval-mode
 * forward too. */
int zf_condnet_backward(zf_condnet_t* handle, const float* gc, float* grad_out, void* stream);

/* Replaces jax.grad(loss_fn) of the notebook's first half (`class DeepSet`:
 * rho(phi(x))) for the network's input as well: zf_condnet_backward plus
 * gx_out (device, (rows of the pending pass, in_dim) fp32, not NULL), which
 * receives d loss / d x — what sends a loss behind this network on into the
 * network in front of it (rho's gx is phi's gc).  grad_out and the kept
 * gradient have the bits zf_condnet_backward gives for the same pass.
 *   without BatchNorm  the first Dense layer's input-gradient GEMM,
 *                      gx = g_0 . W_0^T, written to gx_out;
 *   with BatchNorm     the train-mode reverse with the batch terms,
 *                      gx = rstd * (gUhat - mean(gUhat) - u_hat * mean(gUhat * u_hat)),
 *                      gUhat = gUbn * scale, the means over all rows passed
 *                      (padding rows are in the forward's statistics); the
 *                      two column sums are the ones the scale and bias
 *                      gradients reduce, formed once.
 * No atomics: the same pass gives the same gx bits.  The pending rules are
 * zf_condnet_backward's; a NULL gx_out is ZF_EINVAL with nothing enqueued and
 * the pass still pending.  An eval-mode forward leaves nothing pending: there
 * is no eval-mode input gradient. */
int zf_condnet_backward_input(zf_condnet_t* handle, const float* gc, float* grad_out, float* gx_out, void* stream);

/* Replaces opt.update + optax.apply_updates of `step`: the optimiser chain on
 * grad (device, blob layout; NULL: the last backward's). */
int zf_condnet_apply_gradient(zf_condnet_t* handle, const float* grad, void* stream);

/* Replace the optimiser by a chain, as zf_trainer_set_optim_chain does (same
 * stages, limits and messages).  Synchronises; resets moments and count. */
int zf_condnet_set_optim_chain(zf_condnet_t* handle, const zf_optim_chain* chain,
                               const unsigned char* decay_mask);

/* Copy the blob (parameters + statistics) out / in.  These two, the four
 * optimiser-state entries below, zf_condnet_set_optim_chain and a
 * zf_condnet_set_comm that grows the gather buffer synchronise with the
 * host; no other zf_condnet_* or zf_segment_* entry does.  None captures a
 * graph.  Under a communicator of more than one rank
 * zf_condnet_forward(_shard) in train mode with BatchNorm,
 * zf_condnet_backward and zf_condnet_backward_input communicate
 * (zf_condnet_set_comm); no other entry does. */
int zf_condnet_get_blob(zf_condnet_t* handle, float* blob_host);
int zf_condnet_set_blob(zf_condnet_t* handle, const float* blob_host);

/* The optimiser's state, as zf_trainer_get_opt_slot / _set_opt_slot /
 * _get_opt_scalars / _set_opt_count give and take the trainer's: the same
 * arguments and errors; a handle's optimiser is always a chain (the (n)adamw
 * of zf_condnet_create keeps two slots, mu and nu).  With the blob it is all
 * a run needs to resume.  They synchronise. */
int zf_condnet_get_opt_slot(zf_condnet_t* handle, int slot, float* host_floats);
int zf_condnet_set_opt_slot(zf_condnet_t* handle, int slot, const float* host_floats);
int zf_condnet_get_opt_scalars(zf_condnet_t* handle, int64_t* count, double* learning_rate, double* grad_norm);
int zf_condnet_set_opt_count(zf_condnet_t* handle, int64_t count);

/* ------------------------------------------------------------------------ */
/* RCCL (over xGMI) — the NLL all-reduce of data-parallel log_prob and the  */
/* trainer's all-gather.                                                      */
/* ------------------------------------------------------------------------ */
int zf_rccl_available(void);
int zf_rccl_get_unique_id(char* id128);
int zf_rccl_comm_init(void** comm, int nranks, const char* id128, int rank);
int zf_rccl_allreduce_sum_f64(void* comm, const double* send, double* recv, size_t count,
                              void* stream);
int zf_rccl_comm_destroy(void* comm);
/* zf_allgather_fn over RCCL (ncclAllGather of bytes): comm = ctx. */
int zf_rccl_allgather(void* comm, const void* send, void* recv, size_t bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ZENFLOW_AMD_H */
