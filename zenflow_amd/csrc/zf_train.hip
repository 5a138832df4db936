// Training: train-mode forward with stored activations, the reverse pass
// (RQ spline, conditioner MLP, BatchNorm with batch statistics) and the
// optimiser update, for zenflow.train (src/zenflow/train.py:18-138):
//   loss_fn  (train.py:64-72): -mean(Flow.__call__(x, c, train=True))
//   step     (train.py:80-86): jax.grad -> optax (n)adamw update
// and the gradients with respect to the flow's inputs, which the reference's
// users take by differentiating Flow as a JAX function:
//   train mode  d loss / d c (train.py:64-86 through c; the DeepSetFlow /
//               loss_fn_2 cells of examples/deep_set.ipynb feed c = phi(x)
//               into self.flow(y, c, train=train) and train phi with jax.grad)
//   eval mode   the vector-Jacobian product of log_prob (flow.py:22-48) with
//               respect to x and c (zf_trainer_log_prob_vjp)
// The path is op by op and unfused (a training batch is 10^3-10^5 rows; the
// weights change every step, so the fused inference kernels' packed weight
// layouts would have to be rebuilt each step).  GEMMs are an LDS-tiled fp32
// kernel; everything else is per-row elementwise / per-column reductions.
// All parameters and gradients live in the natural FLAX blob layout of
// zf_flow_plan on the device.
// This file is the trainer itself (zf_trainer, the host logic, the C ABI);
// its kernels are in the headers below, one concern each, all part of this
// one translation unit: zf_gemm.h (GEMMs and the gemm() dispatcher),
// zf_reduce.h (batch reductions, weight gradients), zf_train_kernels.h
// (element-wise kernels) and zf_train_spline.h (RQ-spline rows).  The host
// logic is a handful of passes over the coupling chain, each a loop of the
// per-coupling helpers they share (nsc_dense_fwd, nsc_eval_conditioner,
// spline_reverse, nsc_reverse_mlp, bn_param_grads, bn_eval_reverse,
// latent_vjp_launch, close_gradient):
//   forward   trainer_forward_train, trainer_forward_eval, and
//             trainer_sample_forward (flow.py:50-78 as a differentiable
//             function; its kernels are zf_train_sample.h in zf_sample_grad.hip)
//   reverse   trainer_reverse (train and eval mode), trainer_sample_reverse
//   whole     trainer_body (train-mode forward + loss + trainer_reverse),
//             trainer_vjp_chunk (eval forward + the input gradients)
// behind the entries run_loss_grad / run_step (the eight loss_grad / step
// entries), zf_trainer_log_prob_vjp, zf_trainer_forward / _backward /
// _apply_gradient and zf_trainer_sample_forward / _sample_backward.
#include "zf_gemm.h"
#include "zf_internal.h"
#include "zf_optim.h"
#include "zf_reduce.h"
#include "zf_train_kernels.h"
#include "zf_train_spline.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <map>
#include <vector>

// ============================================================================
struct zf_trainer {
  zf_flow_desc desc;
  int D = 0, C = 0, n_ops = 0;
  int64_t nat_floats = 0;
  int64_t bmax = 0;
  zf_optim_desc opt;
  long long t = 0;  // optimiser step count (host mirror of d_step)
  bool sb_first = false;  // the chain starts with a ShiftBounds (the only place it may stand)
  std::vector<float> sb_modes, sb_prm;  // ShiftBounds pre-transform per dim (colstats)
  float* d_nat = nullptr;
  float* d_grad = nullptr;
  float* d_m = nullptr;
  float* d_v = nullptr;
  unsigned char* d_mask = nullptr;
  // arena: per-op saved activations + scratch
  std::vector<float*> bufs;
  std::vector<int64_t> sizes;
  float* d_state = nullptr;   // [n_ops + 1][bmax][D] states before each op
  std::vector<float*> sp;     // sp[i]: the state before op i (Roll is an index rotation: it aliases its input)
  std::vector<int> rots;      // rots[i]: the column rotation before op i; rots[n_ops]: the latent's
  float* d_c = nullptr;       // [bmax][C] conditioning inputs of the batch
  float* d_bc = nullptr;      // optimiser step count + bias corrections (step_kernel)
  // optimiser chain (zf_trainer_set_optim_chain); off: the (n)adamw of `opt`
  bool chain_on = false;
  zf::ChainArgs cargs{};
  int chain_form = 0;         // kForm*
  int n_slots = 0;
  float max_norm = 0.f;       // clip_by_global_norm (chain_clip)
  bool chain_clip = false, chain_lr = false, chain_adam = false;
  float chain_b1 = 0.f, chain_b2 = 0.f;  // the scale_by_adam stage's, for the bias corrections
  zf_schedule sched{};
  std::vector<void*> opt_bufs;  // what the chain allocated (freed when it is replaced)
  unsigned char* d_dmask = nullptr;
  double* d_nleaf = nullptr;  // leaves of the gradient's sum of squares
  int n_nleaf = 0;
  zf::OptScalars* d_osc = nullptr;
  // zf_trainer_step as one hipGraph per batch size (the body reads only the
  // trainer's own buffers: x and c are copied in before the launch)
  hipStream_t cap = nullptr;
  std::map<int64_t, hipGraphExec_t> graphs;
  std::map<int64_t, hipGraphExec_t> graphs_w;  // the weighted step's (it reads d_w as well)
  bool use_graph = true;
  bool bn_small = true;  // ZF_TRAIN_BN_SMALL=0: always the multi-launch BatchNorm path
  bool splitq = true;    // ZF_TRAIN_SPLITQ=0: never the split-set GEMM (same bits either way)
  float* d_ld = nullptr;      // [bmax]
  float* d_g0 = nullptr;      // [bmax][D]
  float* d_g1 = nullptr;
  float* d_small = nullptr;   // per-column scratch (ShiftBounds min / max)
  float* d_ce = nullptr;      // [bmax] per-row cotangent of the eval-mode VJP / the weighted loss
  float* d_w = nullptr;       // [bmax] per-row weights of the weighted loss
  double* d_leaf = nullptr;   // leaf partials of the BatchNorm sums / loss [kLeafCap][128]
  double* d_leaf2 = nullptr;  // first-level tree roots [kLeafCap / 64][128]
  double* d_ws2 = nullptr;    // first-level roots of the split-K partials
  double* d_roots = nullptr;  // [0,128): tree roots of one reduction; [128]: the loss; [129]: the weight sum
  double* d_rowloss = nullptr;  // [bmax] per-row loss terms
  double* d_g64 = nullptr;    // fp64 gradient accumulator (blob layout)
  // data parallelism: the communicator and its all-gather landing buffer
  zf_comm_desc comm{0, 1, nullptr, nullptr};
  void* d_gath = nullptr;
  int64_t gath_bytes = 0;
  void* d_colws = nullptr;
  float* d_ws = nullptr;      // split-K partials (kWsFloats)
  float* d_split = nullptr;   // split-set GEMM partials (kSplitFloats)
  int64_t colws_bytes = 0;
  struct NscBufs {
    float *U, *Uhat, *Ubn, *P, *gP, *gU, *gA, *gB;
    std::vector<float*> Z, H;
    float *mean, *rstd;
  };
  std::vector<NscBufs> nsc;
  // zf_trainer_forward's pass, waiting for its zf_trainer_backward (kPend*)
  int pend_mode = 0;
  int64_t pend_rows = 0, pend_global = 0;
  // gradients through sampling (zf_trainer_sample_forward / _backward)
  float* d_sm = nullptr;      // [bmax] the pass's row mask: 1 where x and log_q are finite
  float* d_lq = nullptr;      // [bmax] the latent's log-density of the pass's rows
  float* d_gl = nullptr;      // [bmax][D] d log_q's share of d / d z at the latent
  bool sb_ok = false;         // the stored ShiftBounds bounds were seen finite (they only widen)
};

namespace zf {
namespace {

// zf_trainer::pend_mode: no forward pending, or the mode zf_trainer_forward ran in
// (kPendSample: zf_trainer_sample_forward's inverse pass, which only zf_trainer_sample_backward takes)
enum { kPendNone = 0, kPendTrain = 1, kPendEval = 2, kPendSample = 3 };

// Every entry that overwrites the arena drops the pending pass (kPendNone); a forward that ran records its batch.
inline void set_pending(zf_trainer* t, int mode, int64_t rows = 0, int64_t global_rows = 0) {
  t->pend_mode = mode, t->pend_rows = rows, t->pend_global = global_rows;
}

float* dmalloc(zf_trainer* t, int64_t n, int& rc) {
  if (rc) return nullptr;
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, (size_t)(n > 0 ? n : 1) * sizeof(float));
  if (e != hipSuccess) {
    rc = hip_status(e, "zf_trainer alloc");
    return nullptr;
  }
  t->bufs.push_back((float*)p);
  return (float*)p;
}

void nsc_dims(const zf_trainer* t, const zf_op_desc& op, int& dt, int& dc, int& DC, int& S) {
  dt = t->D / 2;
  dc = t->D - dt;
  DC = dc + t->C;
  S = 3 * op.knots - 1;
}

// Destroy every captured step of one cache (the caller has synchronised).
void drop_graphs(std::map<int64_t, hipGraphExec_t>& graphs) {
  for (auto& kv : graphs) (void)hipGraphExecDestroy(kv.second);
  graphs.clear();
}

}  // namespace
}  // namespace zf

extern "C" {

int zf_trainer_create(const zf_flow_desc* desc_in, const float* blob_host, int64_t blob_floats,
                      const unsigned char* param_mask, int64_t batch_max, const zf_optim_desc* opt,
                      zf_trainer_t** out) {
  if (!desc_in || !blob_host || !param_mask || !opt || !out) return zf::einval("NULL argument");
  *out = nullptr;
  zf_flow_desc desc = *desc_in;
  int64_t need = 0;
  int rc = zf_flow_plan(&desc, &need);
  if (rc) return rc;
  if (need != blob_floats) return zf::einval("blob has %lld floats, plan needs %lld", (long long)blob_floats, (long long)need);
  if (batch_max < 1 || batch_max > (1 << 24)) return zf::einval("batch_max outside [1, 2^24]");
  for (int i = 0; i < desc.n_ops; ++i) {
    const zf_op_desc& op = desc.ops[i];
    if (op.kind == ZF_OP_SHIFT_BOUNDS && i != 0)
      return zf::enotsup("training: ShiftBounds is supported only as the first bijector");
    if (op.kind == ZF_OP_NSC && op.knots > zf::kMaxK) return zf::enotsup("training: knots > 64");
    if (op.kind == ZF_OP_NSC && desc.dim - desc.dim / 2 + desc.cond_dim > 64)
      return zf::enotsup("training: more than 64 conditioner inputs");
  }
  zf_trainer* t = new zf_trainer();
  t->desc = desc;
  t->D = desc.dim;
  t->C = desc.cond_dim;
  t->n_ops = desc.n_ops;
  t->nat_floats = need;
  t->bmax = batch_max;
  t->opt = *opt;
  const int64_t B = batch_max, D = desc.dim;
  t->sb_first = desc.n_ops > 0 && desc.ops[0].kind == ZF_OP_SHIFT_BOUNDS;
  if (t->sb_first) {
    const float* row = blob_host + desc.ops[0].off_sb;
    for (int j = 0; j < D; ++j) {
      const int mode = (int)row[8 * j];
      t->sb_modes.push_back((float)mode);
      t->sb_prm.push_back(mode == ZF_SB_LOWER ? row[8 * j + 1] : row[8 * j + 2]);
    }
  }
  rc = ZF_OK;
  t->d_nat = zf::dmalloc(t, need, rc);
  t->d_grad = zf::dmalloc(t, need, rc);
  t->d_m = zf::dmalloc(t, need, rc);
  t->d_v = zf::dmalloc(t, need, rc);
  t->d_mask = (unsigned char*)zf::dmalloc(t, (need + 3) / 4, rc);
  t->d_state = zf::dmalloc(t, (int64_t)(desc.n_ops + 1) * B * D, rc);
  t->d_ld = zf::dmalloc(t, B, rc);
  t->d_g0 = zf::dmalloc(t, B * D, rc);
  t->d_g1 = zf::dmalloc(t, B * D, rc);
  t->d_small = zf::dmalloc(t, 8 * 256, rc);
  t->d_ce = zf::dmalloc(t, B, rc);
  t->d_leaf = (double*)zf::dmalloc(t, 2 * zf::kLeafCap * 128, rc);
  t->d_leaf2 = (double*)zf::dmalloc(t, 2 * (zf::kLeafCap / zf::kMaxLeaves) * 128, rc);
  t->d_ws2 = (double*)zf::dmalloc(t, 2 * (zf::kWsFloats / zf::kMaxLeaves), rc);
  t->d_roots = (double*)zf::dmalloc(t, 2 * 256, rc);
  t->d_rowloss = (double*)zf::dmalloc(t, 2 * B, rc);
  t->d_g64 = (double*)zf::dmalloc(t, 2 * need, rc);
  if (!rc) {
    const hipError_t e = hipMemset(t->d_g64, 0, (size_t)need * sizeof(double));  // 2 need floats
    if (e != hipSuccess) rc = zf::hip_status(e, "zf_trainer_create gradient");
  }
  t->d_ws = zf::dmalloc(t, zf::kWsFloats, rc);
  t->d_split = zf::dmalloc(t, zf::kSplitFloats, rc);
  t->d_c = zf::dmalloc(t, B * (desc.cond_dim > 0 ? desc.cond_dim : 1), rc);
  t->d_bc = zf::dmalloc(t, 4, rc);
  {
    const char* g = std::getenv("ZF_TRAIN_GRAPH");
    t->use_graph = !(g && g[0] == '0');
    const char* bs = std::getenv("ZF_TRAIN_BN_SMALL");
    t->bn_small = !(bs && bs[0] == '0');
    const char* sq = std::getenv("ZF_TRAIN_SPLITQ");
    t->splitq = !(sq && sq[0] == '0');
  }
  if (!rc) {
    hipError_t e = hipStreamCreateWithFlags(&t->cap, hipStreamNonBlocking);
    if (e != hipSuccess) rc = zf::hip_status(e, "zf_trainer_create stream");
  }
  t->colws_bytes = zf_colstats_workspace_bytes(B, 64);
  t->d_colws = zf::dmalloc(t, t->colws_bytes / 4 + 1, rc);
  t->nsc.resize(desc.n_ops);
  for (int i = 0; i < desc.n_ops && !rc; ++i) {
    const zf_op_desc& op = desc.ops[i];
    if (op.kind != ZF_OP_NSC) continue;
    int dt, dc, DC, S;
    zf::nsc_dims(t, op, dt, dc, DC, S);
    zf_trainer::NscBufs& nb = t->nsc[i];
    nb.U = zf::dmalloc(t, B * DC, rc);
    nb.Uhat = zf::dmalloc(t, B * DC, rc);
    nb.Ubn = zf::dmalloc(t, B * DC, rc);
    nb.gU = zf::dmalloc(t, B * DC, rc);
    nb.P = zf::dmalloc(t, B * dt * S, rc);
    nb.gP = zf::dmalloc(t, B * dt * S, rc);
    int hmax = 0;
    for (int l = 0; l < op.n_hidden; ++l) {
      nb.Z.push_back(zf::dmalloc(t, B * op.hidden[l], rc));
      nb.H.push_back(zf::dmalloc(t, B * op.hidden[l], rc));
      hmax = op.hidden[l] > hmax ? op.hidden[l] : hmax;
    }
    nb.gA = zf::dmalloc(t, B * hmax, rc);
    nb.gB = zf::dmalloc(t, B * hmax, rc);
    nb.mean = zf::dmalloc(t, DC, rc);
    nb.rstd = zf::dmalloc(t, DC, rc);
  }
  t->d_w = zf::dmalloc(t, B, rc);  // last: the buffers above keep the places they had without it
  t->d_sm = zf::dmalloc(t, B, rc);  // the sampling pass's, after it for the same reason
  t->d_lq = zf::dmalloc(t, B, rc);
  t->d_gl = zf::dmalloc(t, B * D, rc);
  hipError_t e = hipSuccess;
  if (!rc) e = hipMemcpy(t->d_nat, blob_host, need * sizeof(float), hipMemcpyHostToDevice);
  if (!rc && e == hipSuccess) e = hipMemcpy(t->d_mask, param_mask, need, hipMemcpyHostToDevice);
  if (!rc && e == hipSuccess) e = hipMemset(t->d_m, 0, need * sizeof(float));
  if (!rc && e == hipSuccess) e = hipMemset(t->d_v, 0, need * sizeof(float));
  if (!rc && e == hipSuccess) e = hipMemset(t->d_bc, 0, 4 * sizeof(float));
  if (!rc && e != hipSuccess) rc = zf::hip_status(e, "zf_trainer_create");
  if (rc) {
    zf_trainer_destroy(t);
    return rc;
  }
  // the coupling chain's state pointers and rotations depend on desc and bmax only
  t->sp.assign(desc.n_ops + 1, t->d_state);
  t->rots.assign(desc.n_ops + 1, 0);
  for (int i = 0; i < desc.n_ops; ++i) {
    const bool roll = desc.ops[i].kind == ZF_OP_ROLL;
    t->sp[i + 1] = roll ? t->sp[i] : t->d_state + (int64_t)(i + 1) * B * D;
    t->rots[i + 1] = roll ? zf::pmodi(t->rots[i] - desc.ops[i].shift, (int)D) : t->rots[i];
  }
  *out = t;
  return ZF_OK;
}

int zf_trainer_destroy(zf_trainer_t* t) {
  if (!t) return ZF_OK;
  (void)hipDeviceSynchronize();
  zf::drop_graphs(t->graphs);
  zf::drop_graphs(t->graphs_w);
  if (t->cap) (void)hipStreamDestroy(t->cap);
  for (float* p : t->bufs) (void)hipFree(p);
  for (void* p : t->opt_bufs) (void)hipFree(p);
  if (t->d_gath) (void)hipFree(t->d_gath);
  delete t;
  return ZF_OK;
}

int zf_trainer_set_comm(zf_trainer_t* t, const zf_comm_desc* comm) {
  if (!t) return zf::einval("trainer is NULL");
  zf_comm_desc c{0, 1, nullptr, nullptr};
  if (comm) c = *comm;
  if (c.world < 1 || c.rank < 0 || c.rank >= c.world) return zf::einval("bad rank %d / world %d", c.rank, c.world);
  if (c.world > zf::kMaxLeaves) return zf::enotsup("training: more than 64 ranks");
  if (c.world > 1 && !c.allgather) return zf::einval("communicator without allgather");
  // the gather buffer only grows (largest exchange: the fp64 gradient of
  // every rank), and stays allocated while the communicator is cleared for a
  // one-device step (train(): a batch with fewer rows than ranks, once per
  // epoch), so clearing / restoring it costs no device sync or allocation
  const int64_t need =
      c.world > 1 ? std::max<int64_t>(t->nat_floats, 256) * (int64_t)sizeof(double) * c.world : 0;
  if (need > t->gath_bytes) {
    ZF_TRY_HIP(hipDeviceSynchronize());
    if (t->d_gath) (void)hipFree(t->d_gath);
    t->d_gath = nullptr;
    t->gath_bytes = 0;
    ZF_TRY_HIP(hipMalloc(&t->d_gath, (size_t)need));
    t->gath_bytes = need;
  }
  t->comm = c;
  return ZF_OK;
}

}  // extern "C"

namespace zf {
namespace {

// One loss_grad / step call, as the widest C entry states it: this rank's
// rows of a global batch, their weights (NULL: the unweighted loss) and the
// outputs (grad NULL: the trainer's own; gc NULL or C == 0: no d loss / d c).
struct BatchArgs {
  const float *x, *c, *w;
  int64_t rows, global_rows;
  int update_stats;
  double* loss;
  float *grad, *gc;
  hipStream_t stream;
};

// What check_batch holds a batch to.
enum BatchRule {
  kBatchShard,    // this rank's shard of global_rows rows; on one device global_rows == rows
  kBatchSample,   // latent rows z of a sampling pass: it has no batch statistics, so on one device a larger
                  // global_rows only declares the rows a micro-batch of that batch (it picks the GEMM forms
                  // and the leaf layout)
  kBatchChunked,  // N rows of zf_trainer_log_prob_vjp, taken bmax at a time: no upper bound
};

// Everything that can be wrong with a batch, before anything is enqueued.
int check_batch(const zf_trainer_t* t, const BatchArgs& a, BatchRule rule = kBatchShard) {
  if (!t) return einval("trainer is NULL");
  if (rule == kBatchChunked) {
    if (a.rows < 1) return einval("N must be at least 1");
  } else if (a.rows < 1 || a.rows > t->bmax) {
    return einval("batch %lld outside [1, %lld]", (long long)a.rows, (long long)t->bmax);
  }
  if (!a.x) return einval("%s is NULL", rule == kBatchSample ? "z" : "x");
  if (t->C > 0 && !a.c) return einval("flow is conditional but c is NULL");
  if (a.global_rows < a.rows || (rule == kBatchShard && t->comm.world == 1 && a.global_rows != a.rows))
    return einval("global_rows %lld vs rows %lld (world %d)", (long long)a.global_rows, (long long)a.rows,
                  t->comm.world);
  return ZF_OK;
}

// Copy B64 checked rows into the trainer's buffers (state 0, d_c, and the
// rows' weights into d_w when the loss is weighted).
int trainer_stage(zf_trainer_t* t, const float* x, const float* c, const float* w, int64_t B64, hipStream_t st) {
  ZF_TRY_HIP(hipMemcpyAsync(t->d_state, x, (size_t)B64 * t->D * sizeof(float), hipMemcpyDeviceToDevice, st));
  if (t->C > 0)
    ZF_TRY_HIP(hipMemcpyAsync(t->d_c, c, (size_t)B64 * t->C * sizeof(float), hipMemcpyDeviceToDevice, st));
  if (w) ZF_TRY_HIP(hipMemcpyAsync(t->d_w, w, (size_t)B64 * sizeof(float), hipMemcpyDeviceToDevice, st));
  return ZF_OK;
}

inline double* loss_slot(zf_trainer_t* t) { return t->d_roots + 128; }
inline double* wsum_slot(zf_trainer_t* t) { return t->d_roots + 129; }  // the weighted loss's sum of weights

// Data parallelism: this rank's tree roots (n doubles, in place) -> the
// global ones: all-gather every rank's roots, combine them by the top of the
// leaf tree (tree_n over ranks).  Nothing to do on one device.
int dp_combine(zf_trainer_t* t, double* roots, long long n, hipStream_t st) {
  const int W = t->comm.world;
  if (W <= 1) return ZF_OK;
  if ((int64_t)n * (int64_t)sizeof(double) * W > t->gath_bytes) return einval("all-gather buffer too small");
  const int rc = t->comm.allgather(t->comm.ctx, roots, t->d_gath, (size_t)n * sizeof(double), st);
  if (rc) return rc;
  return launch_tree_cols((const double*)t->d_gath, W, n, roots, st);
}

// ---- The per-coupling helpers the passes share.  i is the coupling's place in
// the chain: its op is t->desc.ops[i], its activations t->nsc[i], its column
// rotation t->rots[i].  B: this rank's rows; Bg: the batch that picks the GEMM
// forms and the leaf layouts (the global batch; the chunk itself in
// trainer_vjp_chunk) ----

// The Dense chain of one coupling's conditioner: nb.Ubn -> Z[l], H[l] = act(Z[l]) -> nb.P
// (dt * S raw spline parameters per row).
int nsc_dense_fwd(zf_trainer_t* t, const zf_op_desc& op, zf_trainer::NscBufs& nb, long long Bg, int B, int DC,
                  int out_last, hipStream_t st) {
  const float* nat = t->d_nat;
  const float* in = nb.Ubn;
  int in_w = DC;
  for (int l = 0; l <= op.n_hidden; ++l) {
    const bool last = (l == op.n_hidden);
    const int out_w = last ? out_last : op.hidden[l];
    const int rc = gemm(false, Bg, B, out_w, in_w, in, in_w, nat + op.off_w[l], out_w, last ? nb.P : nb.Z[l], out_w, st,
                        kEpiBias, nat + op.off_b[l], last ? nullptr : nb.H[l], nullptr, op.act,
                        t->splitq ? t->d_split : nullptr, kSplitFloats);
    if (rc) return rc;
    if (!last) {
      in = nb.H[l];
      in_w = out_w;
    }
  }
  return ZF_OK;
}

// One coupling's conditioner in eval mode, from the state that holds its
// conditioning columns: BatchNorm on the stored mean / var (nb.Ubn, nb.rstd;
// keep_uhat: also nb.Uhat, which the BatchNorm scale gradient reads, Ubn has
// the same bits either way), then the Dense chain to nb.P.
int nsc_eval_conditioner(zf_trainer_t* t, int i, const float* state_in, bool keep_uhat, int B, long long Bg,
                         hipStream_t st) {
  const zf_op_desc& op = t->desc.ops[i];
  zf_trainer::NscBufs& nb = t->nsc[i];
  int dt, dc, DC, S;
  nsc_dims(t, op, dt, dc, DC, S);
  const float* bn = t->d_nat + op.off_bn;
  if (keep_uhat) {
    hipLaunchKernelGGL(bn_eval_fwd_uhat_kernel, dim3(blocks_for((int64_t)B * DC)), dim3(256), 0, st, state_in,
                       (const float*)t->d_c, bn, nb.Uhat, nb.Ubn, nb.rstd, B, t->D, t->C, dt, dc, t->rots[i]);
    ZF_CHECK_LAUNCH("bn_eval_fwd_uhat_kernel");
  } else {
    hipLaunchKernelGGL(bn_eval_fwd_kernel, dim3(blocks_for((int64_t)B * DC)), dim3(256), 0, st, state_in,
                       (const float*)t->d_c, bn, nb.Ubn, nb.rstd, B, t->D, t->C, dt, dc, t->rots[i]);
    ZF_CHECK_LAUNCH("bn_eval_fwd_kernel");
  }
  return nsc_dense_fwd(t, op, nb, Bg, B, DC, dt * S, st);
}

// The reverse of one coupling's spline: g = d / d (state i + 1) -> g_prev
// (the transformed columns of d / d (state i)) and nb.gP.  ce: d / d log_det
// per row (NULL: gl for every row).
int spline_reverse(zf_trainer_t* t, int i, const float* g, float* g_prev, const float* ce, float gl, int B,
                   hipStream_t st) {
  const zf_op_desc& op = t->desc.ops[i];
  zf_trainer::NscBufs& nb = t->nsc[i];
  const int D = t->D, dt = D / 2, r = t->rots[i];
  return ce ? spline_bwd_launch<true>(t->sp[i], nb.P, g, 0.f, g_prev, nb.gP, B, D, dt, op.knots, r, ce, st)
            : spline_bwd_launch<false>(t->sp[i], nb.P, g, gl, g_prev, nb.gP, B, D, dt, op.knots, r, nullptr, st);
}

// The reverse of one coupling's Dense chain, last layer first, from nb.gP =
// d / d (raw spline parameters) to nb.gU = d / d Ubn.  gout (out_w wide) is
// d / d (layer l's output); layer l's GEMM writes d / d (its input) through
// the activation of layer l - 1 to gin: nb.gU for layer 0, else nb.gA / nb.gB
// in turn.  wq (NULL: no weight gradients, trainer_vjp_chunk): before each
// layer's GEMM, its dW_l = hin^T . gout and db_l = colsum(gout) are queued
// into the fp64 gradient.
int nsc_reverse_mlp(zf_trainer_t* t, int i, int B, long long Bg, WgradQueue* wq, hipStream_t st) {
  const zf_op_desc& op = t->desc.ops[i];
  zf_trainer::NscBufs& nb = t->nsc[i];
  int dt, dc, DC, S;
  nsc_dims(t, op, dt, dc, DC, S);
  const float* gout = nb.gP;
  int out_w = dt * S, which = 0, rc;
  for (int l = op.n_hidden; l >= 0; --l) {
    const int in_w = l == 0 ? DC : op.hidden[l - 1];
    float* const gin = l == 0 ? nb.gU : (which ? nb.gB : nb.gA);
    if (wq) {
      const float* hin = l == 0 ? nb.Ubn : nb.H[l - 1];
      // leaves capped by the split-K workspace (a power of two, the same on every rank)
      const int cap = pow2floor(std::min<int64_t>(kLeafCap, std::max<int64_t>(1, kWsFloats / ((int64_t)(in_w + 1) * out_w))));
      rc = wgrad_deferred(*wq, in_w, out_w, B, leaves_for(B, Bg, t->comm.world, cap), hin, gout,
                          t->d_g64 + op.off_w[l], t->d_g64 + op.off_b[l], t->d_ws, t->d_ws2, st);
      if (rc) return rc;
      if ((rc = wgrad_before_write(*wq, gin, st))) return rc;  // a deferred dW GEMM still reads it
    }
    rc = gemm(true, Bg, B, in_w, out_w, gout, out_w, t->d_nat + op.off_w[l], out_w, gin, in_w, st,
              l > 0 ? kEpiDSwish : kEpiNone, nullptr, nullptr, l > 0 ? nb.Z[l - 1] : nullptr, op.act,
              t->splitq ? t->d_split : nullptr, kSplitFloats);
    if (rc) return rc;
    gout = gin;
    out_w = in_w;
    which ^= 1;
  }
  return ZF_OK;
}

// One coupling's BatchNorm scale / bias gradient from nb.gU = d / d Ubn: the
// sums of gUbn and gUbn * Uhat over this rank's rows, leaves -> tree, copied
// into the fp64 gradient.  The roots stay in d_roots ([0, DC): bias,
// [DC, 2 DC): scale), where the train-mode reverse goes on with them.
int bn_param_grads(zf_trainer_t* t, int i, const Leaves& lbn, int B, hipStream_t st) {
  const zf_op_desc& op = t->desc.ops[i];
  zf_trainer::NscBufs& nb = t->nsc[i];
  int dt, dc, DC, S;
  nsc_dims(t, op, dt, dc, DC, S);
  double* gbn = t->d_g64 + op.off_bn;
  hipLaunchKernelGGL(leaf_colsums_kernel, dim3(blocks_for((int64_t)lbn.n * DC)), dim3(256), 0, st, nb.gU, nb.Uhat, B,
                     DC, lbn.rows, lbn.n, t->d_leaf);
  ZF_CHECK_LAUNCH("leaf_colsums_kernel");
  const int rc = launch_tree_cols(t->d_leaf, lbn.n, 2 * DC, t->d_roots, st, t->d_leaf2);
  if (rc) return rc;
  ZF_TRY_HIP(hipMemcpyAsync(gbn + 3 * DC, t->d_roots, DC * sizeof(double), hipMemcpyDeviceToDevice, st));
  ZF_TRY_HIP(hipMemcpyAsync(gbn + 2 * DC, t->d_roots + DC, DC * sizeof(double), hipMemcpyDeviceToDevice, st));
  return ZF_OK;
}

// The reverse through one coupling's BatchNorm on the stored statistics (no
// batch terms): gU = gUbn scale rstd on the rows whose mask entry is not zero,
// its state columns added into g_out, its condition columns into gc (NULL:
// none; gc_assign: stored, not added).
int bn_eval_reverse(zf_trainer_t* t, int i, const float* mask, float* g_out, float* gc, int gc_assign, int B,
                    hipStream_t st) {
  const zf_op_desc& op = t->desc.ops[i];
  zf_trainer::NscBufs& nb = t->nsc[i];
  int dt, dc, DC, S;
  nsc_dims(t, op, dt, dc, DC, S);
  hipLaunchKernelGGL(bn_eval_bwd_kernel, dim3(blocks_for((int64_t)B * DC)), dim3(256), 0, st, (const float*)nb.gU,
                     (const float*)(t->d_nat + op.off_bn + 2 * DC), (const float*)nb.rstd, mask, g_out, gc, gc_assign,
                     B, t->D, t->C, dt, dc, t->rots[i]);
  ZF_CHECK_LAUNCH("bn_eval_bwd_kernel");
  return ZF_OK;
}

// A chain without a coupling met nothing that assigns gc: the pass's result does not depend on c.
int gc_zero_unassigned(zf_trainer_t* t, float* gc, int gc_assign, int B, hipStream_t st) {
  if (gc && gc_assign) ZF_TRY_HIP(hipMemsetAsync(gc, 0, (size_t)B * t->C * sizeof(float), st));
  return ZF_OK;
}

// The latent's log-density of the rows in the last state on top of d_ld, with
// nan_to_num (lp_out, or NULL); d_ce = cot (NULL: ones) where it is finite
// before nan_to_num, 0 elsewhere; g_out = ce . d latent_lp / dz.
int latent_vjp_launch(zf_trainer_t* t, int B, const float* cot, float* lp_out, float* g_out, hipStream_t st) {
  const LatentConsts lc(t->desc);
  hipLaunchKernelGGL(latent_vjp_kernel, dim3(blocks_for(B)), dim3(256), 0, st, t->sp[t->n_ops], t->d_ld, cot, B, t->D,
                     t->rots[t->n_ops], lc.lt, lc.a, lc.betac, lc.tnm, lp_out, t->d_ce, g_out);
  ZF_CHECK_LAUNCH("latent_vjp_kernel");
  return ZF_OK;
}

// The end of a reverse pass: the fp64 gradient (all ranks' shares, tree over
// ranks) -> fp32 G.  step_in_cast (one device, an (n)adamw update follows):
// the cast also advances the optimiser's step counter.
int close_gradient(zf_trainer_t* t, float* G, bool step_in_cast, hipStream_t st) {
  const int W = t->comm.world;
  if (W > 1) {
    const int rc = t->comm.allgather(t->comm.ctx, t->d_g64, t->d_gath, (size_t)t->nat_floats * sizeof(double), st);
    if (rc) return rc;
#define ZF_L(NM) hipLaunchKernelGGL((tree_cols_cast_kernel<NM>), dim3(blocks_for(t->nat_floats)), dim3(256), 0, st, \
                                    (const double*)t->d_gath, W, (long long)t->nat_floats, G)
    ZF_NMAX_DISPATCH(W, ZF_L);
#undef ZF_L
    ZF_CHECK_LAUNCH("tree_cols_cast_kernel");
  } else {
    hipLaunchKernelGGL(cast_f64_f32_kernel, dim3(blocks_for(t->nat_floats)), dim3(256), 0, st, t->d_g64,
                       (long long)t->nat_floats, G, step_in_cast ? t->d_bc : nullptr, t->opt.b1, t->opt.b2);
    ZF_CHECK_LAUNCH("cast_f64_f32_kernel");
  }
  return ZF_OK;
}

// ---- The forward passes ----

// The train-mode forward of the staged batch of B rows (this rank's shard of a
// global batch of Bg rows): batch statistics (exchanged over the ranks), the
// running-statistics update when update_stats is set, every activation the
// reverse pass reads kept in the arena, the log-det in d_ld.  The first half
// of trainer_body and of zf_trainer_forward(train = 1).
int trainer_forward_train(zf_trainer_t* t, int B, long long Bg, int update_stats, hipStream_t st) {
  const int D = t->D, C = t->C, W = t->comm.world;
  const float* c = t->d_c;
  const zf_flow_desc& desc = t->desc;
  float* nat = t->d_nat;
  const std::vector<int>& rots = t->rots;
  auto state = [&](int i) { return t->sp[i]; };
  // a leading ShiftBounds sets ld itself (sb_forward_kernel, first)
  if (!t->sb_first) ZF_TRY_HIP(hipMemsetAsync(t->d_ld, 0, (size_t)B * sizeof(float), st));
  const Leaves lbn = leaves_for(B, Bg, W, kBnLeafCap);
  // the single-block BatchNorm kernels have no exchange point (one device only)
  const bool small_ok = W == 1 && t->bn_small;
  int rc;
  for (int i = 0; i < desc.n_ops; ++i) {
    const zf_op_desc& op = desc.ops[i];
    if (op.kind == ZF_OP_ROLL) continue;  // an index rotation: rots[i + 1]
    const int rot = rots[i];
    float* sin = state(i);
    float* sout = state(i + 1);
    if (op.kind == ZF_OP_SHIFT_BOUNDS) {
      float* sb = nat + op.off_sb;
      // batch min / max of the (safe_log-transformed) columns (first op: rot == 0)
      rc = zf_colstats(sin, B, D, D, 0, t->sb_modes.data(), t->sb_prm.data(), t->d_small, t->d_small + 64,
                       nullptr, nullptr, t->d_colws, st);
      if (rc) return rc;
      if (W > 1) {  // min / max over all ranks (exact in any order)
        rc = t->comm.allgather(t->comm.ctx, t->d_small, t->d_gath, 128 * sizeof(float), st);
        if (rc) return rc;
        hipLaunchKernelGGL(minmax_ranks_kernel, dim3(1), dim3(64), 0, st, (const float*)t->d_gath, W, D,
                           t->d_small, t->d_small + 64);
        ZF_CHECK_LAUNCH("minmax_ranks_kernel");
      }
      hipLaunchKernelGGL(zf::sb_forward_kernel, dim3(zf::blocks_for(B)), dim3(256), 0, st, sin, sout, t->d_ld, sb, B,
                         D, rot, (const float*)t->d_small, (const float*)(t->d_small + 64), update_stats,
                         i == 0 ? 1 : 0);
      ZF_CHECK_LAUNCH("sb_forward_kernel");
    } else if (op.kind == ZF_OP_NSC) {
      int dt, dc, DC, S;
      zf::nsc_dims(t, op, dt, dc, DC, S);
      zf_trainer::NscBufs& nb = t->nsc[i];
      float* bn = nat + op.off_bn;  // [mean, var, scale, bias]
      if (small_ok && (long long)B * DC <= zf::kBnSmall) {
        hipLaunchKernelGGL(zf::bn_fwd_small, dim3(1), dim3(1024), 0, st, sin, c, nb.Uhat, nb.Ubn, bn, nb.mean,
                           nb.rstd, B, D, C, dt, dc, rot, lbn.n, lbn.rows, update_stats);
        ZF_CHECK_LAUNCH("bn_fwd_small");
      } else {
        hipLaunchKernelGGL(zf::gather_u_kernel, dim3(zf::blocks_for((int64_t)B * DC)), dim3(256), 0, st, sin, c,
                           nb.U, B, D, C, dt, dc, rot);
        ZF_CHECK_LAUNCH("gather_u_kernel");
        // column sums / sums of squares: leaves -> tree -> (ranks) -> statistics
        hipLaunchKernelGGL(leaf_colsums_kernel, dim3(blocks_for((int64_t)lbn.n * DC)), dim3(256), 0, st, nb.U,
                           nullptr, B, DC, lbn.rows, lbn.n, t->d_leaf);
        ZF_CHECK_LAUNCH("leaf_colsums_kernel");
        if ((rc = launch_tree_cols(t->d_leaf, lbn.n, 2 * DC, t->d_roots, st, t->d_leaf2))) return rc;
        if ((rc = dp_combine(t, t->d_roots, 2 * DC, st))) return rc;
        hipLaunchKernelGGL(zf::bn_stats_kernel, dim3(1), dim3(64), 0, st, t->d_roots, t->d_roots + DC, Bg, DC, bn,
                           nb.mean, nb.rstd, update_stats);
        ZF_CHECK_LAUNCH("bn_stats_kernel");
        hipLaunchKernelGGL(zf::bn_apply_kernel, dim3(zf::blocks_for((int64_t)B * DC)), dim3(256), 0, st, nb.U,
                           nb.mean, nb.rstd, bn + 2 * DC, bn + 3 * DC, nb.Uhat, nb.Ubn, B, DC);
        ZF_CHECK_LAUNCH("bn_apply_kernel");
      }
      if ((rc = nsc_dense_fwd(t, op, nb, Bg, B, DC, dt * S, st))) return rc;
      if ((rc = spline_fwd_launch(sin, sout, nb.P, t->d_ld, B, D, dt, op.knots, rot, st))) return rc;
    } else {
      return zf::einval("op %d: unknown kind", i);
    }
  }
  return ZF_OK;
}

// The eval-mode forward of the staged batch of B rows (BatchNorm on the stored
// mean / var, ShiftBounds on the stored bounds: rows are independent, nothing
// is exchanged), activations kept in the arena, the log-det in d_ld.  Bg picks
// the GEMM forms.  keep_uhat: also every coupling's nb.Uhat (zf_trainer_forward).
int trainer_forward_eval(zf_trainer_t* t, int B, long long Bg, bool keep_uhat, hipStream_t st) {
  const zf_flow_desc& desc = t->desc;
  const std::vector<float*>& sp = t->sp;
  if (!t->sb_first) ZF_TRY_HIP(hipMemsetAsync(t->d_ld, 0, (size_t)B * sizeof(float), st));
  int rc;
  for (int i = 0; i < desc.n_ops; ++i) {
    const zf_op_desc& op = desc.ops[i];
    if (op.kind == ZF_OP_ROLL) continue;  // an index rotation: rots[i + 1]
    if (op.kind == ZF_OP_SHIFT_BOUNDS) {  // i == 0 (zf_trainer_create)
      hipLaunchKernelGGL(sb_eval_fwd_kernel, dim3(blocks_for(B)), dim3(256), 0, st, sp[i], sp[i + 1], t->d_ld,
                         (const float*)(t->d_nat + op.off_sb), B, t->D);
      ZF_CHECK_LAUNCH("sb_eval_fwd_kernel");
    } else if (op.kind == ZF_OP_NSC) {
      if ((rc = nsc_eval_conditioner(t, i, sp[i], keep_uhat, B, Bg, st))) return rc;
      rc = spline_fwd_launch(sp[i], sp[i + 1], t->nsc[i].P, t->d_ld, B, t->D, t->D / 2, op.knots, t->rots[i], st);
      if (rc) return rc;
    } else {
      return einval("op %d: unknown kind", i);
    }
  }
  return ZF_OK;
}

// x = bijector.inverse(z, c) as a differentiable op (flow.py:76-77): eval mode
// only, BatchNorm on the stored statistics (bijectors.py:367-371), ShiftBounds
// on the stored bounds (:210-240).  The latent rows are staged in the last
// state and the chain is walked from the last op to the first; for a coupling
// the conditioning columns are the same on both sides, so the conditioner runs
// on the op's input state of this pass (nsc_eval_conditioner, the eval
// forward's own launches) and the spline inverse follows.  The states end up
// where a forward pass on x would leave them, the activations in t->nsc[i];
// d_ld collects every op's forward log-det at the inverse's own intermediate,
// d_sm the row mask.
int trainer_sample_forward(zf_trainer_t* t, int B, long long Bg, float* x_out, float* lq_out, hipStream_t st) {
  const int D = t->D;
  const zf_flow_desc& desc = t->desc;
  const std::vector<float*>& sp = t->sp;
  ZF_TRY_HIP(hipMemsetAsync(t->d_ld, 0, (size_t)B * sizeof(float), st));
  ZF_TRY_HIP(hipMemsetAsync(t->d_sm, 0, (size_t)B * sizeof(float), st));
  // the latent's log-density (on the zero log-det) and its finite flag; the gz
  // output is rewritten by the reverse pass
  int rc = latent_vjp_launch(t, B, nullptr, t->d_lq, t->d_g0, st);
  if (rc) return rc;
  for (int i = desc.n_ops - 1; i >= 0; --i) {
    const zf_op_desc& op = desc.ops[i];
    if (op.kind == ZF_OP_ROLL || op.kind == ZF_OP_SHIFT_BOUNDS) continue;  // Roll: index map; ShiftBounds (first op): below
    if (op.kind != ZF_OP_NSC) return einval("op %d: unknown kind", i);
    if ((rc = nsc_eval_conditioner(t, i, sp[i + 1], true, B, Bg, st))) return rc;
    rc = spline_inv_ld_launch(sp[i + 1], sp[i], t->nsc[i].P, t->d_ld, t->d_sm, B, D, D / 2, op.knots, t->rots[i], st);
    if (rc) return rc;
  }
  return sb_eval_inv_launch(sp[t->sb_first ? 1 : 0], sp[0], x_out, t->sb_first ? t->d_nat + desc.ops[0].off_sb : nullptr,
                            t->d_ld, t->d_lq, t->d_ce, t->d_sm, lq_out, B, D, st);
}

// ---- The reverse passes: seed, per coupling the spline's reverse,
// nsc_reverse_mlp and the reverse through BatchNorm, then close_gradient.
// The fp64 gradient needs no clearing per pass: every parameter entry is
// assigned (the weight-gradient trees, the BatchNorm scale / bias gradients)
// and the non-parameter entries (batch statistics, ShiftBounds rows) stay at
// the zeros written once at zf_trainer_create ----

// How trainer_reverse seeds and closes the reverse pass.
struct ReverseArgs {
  bool rowce;         // d / d log_det of row b is d_ce[b] (else -1 / Bg for every row)
  bool eval;          // the forward ran on the stored statistics (zf_trainer_forward, train = 0)
  float* gc;          // this rank's (B, C) rows of d / d c, or NULL
  float* G;           // the fp32 gradient (blob layout)
  bool step_in_cast;  // one device, an (n)adamw update follows: the cast also steps
};

// The reverse pass from d_g0 = d / d latent (and d_ce with ra.rowce) through
// the activations a forward left in the arena, to the fp32 gradient ra.G: the
// second half of trainer_body and of zf_trainer_backward.  ra.eval (the
// forward ran on the stored statistics, nb.Uhat kept): the same spline
// reverse, MLP reverse and BatchNorm scale / bias gradients; the reverse
// through BatchNorm without its batch terms (bn_eval_reverse), so only the
// gradient gather at the end exchanges anything over the ranks.
int trainer_reverse(zf_trainer_t* t, int B, long long Bg, const ReverseArgs& ra, hipStream_t st) {
  const int D = t->D, C = t->C, W = t->comm.world;
  float* const gc = C > 0 ? ra.gc : nullptr;
  const zf_flow_desc& desc = t->desc;
  const Leaves lbn = leaves_for(B, Bg, W, kBnLeafCap);
  const bool small_ok = W == 1 && t->bn_small && !ra.eval;
  float* g = t->d_g0;
  float* g_prev = t->d_g1;
  int rc;
  const float gl = -1.0f / (float)Bg;  // d loss / d log_det of every op and row
  zf::WgradQueue wq;
  wq.tb.count = 0;
  wq.gq.count = 0;
  int gc_assign = 1;  // the first coupling met (the last of the chain) assigns gc
  for (int i = desc.n_ops - 1; i >= 0; --i) {
    const zf_op_desc& op = desc.ops[i];
    if (op.kind == ZF_OP_ROLL || op.kind == ZF_OP_SHIFT_BOUNDS) continue;  // Roll: index map; SB: first op
    int dt, dc, DC, S;
    zf::nsc_dims(t, op, dt, dc, DC, S);
    zf_trainer::NscBufs& nb = t->nsc[i];
    const int r = t->rots[i];
    if ((rc = spline_reverse(t, i, g, g_prev, ra.rowce ? t->d_ce : nullptr, gl, B, st))) return rc;
    if ((rc = nsc_reverse_mlp(t, i, B, Bg, &wq, st))) return rc;
    // BatchNorm: gU holds d loss / d Ubn
    float* bn = t->d_nat + op.off_bn;
    if (small_ok && (long long)B * DC <= zf::kBnSmall) {
      double* gbn = t->d_g64 + op.off_bn;
      hipLaunchKernelGGL(zf::bn_bwd_small, dim3(1), dim3(1024), 0, st, nb.gU, nb.Uhat, bn + 2 * DC, nb.rstd,
                         gbn + 2 * DC, gbn + 3 * DC, g_prev, B, D, C, dt, dc, r, lbn.n, lbn.rows, gc, gc_assign);
      ZF_CHECK_LAUNCH("bn_bwd_small");
    } else if (ra.eval) {
      // this rank's share of the scale / bias gradient (rows with ce == 0 hold zeros)
      if ((rc = bn_param_grads(t, i, lbn, B, st))) return rc;
      if ((rc = bn_eval_reverse(t, i, t->d_ce, g_prev, gc, gc_assign, B, st))) return rc;
    } else {
      // this rank's share of the scale / bias gradient; its roots -> (ranks) ->
      // the reverse formula's global sums
      if ((rc = bn_param_grads(t, i, lbn, B, st))) return rc;
      if ((rc = dp_combine(t, t->d_roots, 2 * DC, st))) return rc;
      // gU := d loss / d U, in place (reads each element before writing it)
      hipLaunchKernelGGL(zf::bn_bwd_kernel, dim3(zf::blocks_for((int64_t)B * DC)), dim3(256), 0, st, nb.gU,
                         nb.Uhat, bn + 2 * DC, nb.rstd, t->d_roots, t->d_roots + DC, nb.gU, B, Bg, DC);
      ZF_CHECK_LAUNCH("bn_bwd_kernel");
      hipLaunchKernelGGL(zf::scatter_gu_kernel, dim3(zf::blocks_for((int64_t)B * dc)), dim3(256), 0, st, nb.gU,
                         g_prev, B, D, C, dt, dc, r);
      ZF_CHECK_LAUNCH("scatter_gu_kernel");
      if (gc) {
        hipLaunchKernelGGL(zf::gather_gc_kernel, dim3(zf::blocks_for((int64_t)B * C)), dim3(256), 0, st, nb.gU, gc, B,
                           C, dc, gc_assign);
        ZF_CHECK_LAUNCH("gather_gc_kernel");
      }
    }
    gc_assign = 0;
    std::swap(g, g_prev);
  }
  if ((rc = zf::wgrad_flush(wq, st))) return rc;
  if ((rc = gc_zero_unassigned(t, gc, gc_assign, B, st))) return rc;
  return close_gradient(t, ra.G, ra.step_in_cast, st);
}

// trainer_sample_forward's reverse: from gx = d L / d x (and glq = d L / d log_q,
// NULL: zeros) of this rank's rows to the fp32 gradient G, gz and gc.  Ops
// from first to last: the spline inverse's reverse, then the ra.eval sequence
// of trainer_reverse with the pass's row mask in place of ce.
int trainer_sample_reverse(zf_trainer_t* t, int B, long long Bg, const float* gx, const float* glq, float* G,
                           float* gz, float* gc_out, hipStream_t st) {
  const int D = t->D;
  float* const gc = t->C > 0 ? gc_out : nullptr;
  const zf_flow_desc& desc = t->desc;
  const std::vector<float*>& sp = t->sp;
  const Leaves lbn = leaves_for(B, Bg, t->comm.world, kBnLeafCap);
  int rc;
  // d L / d log_q per row: where log_q is finite (latent_vjp_kernel's rule, on
  // the whole chain's log-det) and the row counts; its share of gz
  if (glq && (rc = latent_vjp_launch(t, B, glq, nullptr, t->d_gl, st))) return rc;
  if ((rc = sample_mask_cot_launch(glq ? t->d_ce : nullptr, t->d_sm, t->d_ce, B, st))) return rc;
  float* g = t->d_g0;
  float* g_next = t->d_g1;
  rc = sb_eval_inv_bwd_launch(sp[t->sb_first ? 1 : 0], gx, t->d_ce, t->d_sm,
                              t->sb_first ? t->d_nat + desc.ops[0].off_sb : nullptr, g, B, D, st);
  if (rc) return rc;
  zf::WgradQueue wq;
  wq.tb.count = 0;
  wq.gq.count = 0;
  int gc_assign = 1;  // the first coupling met assigns gc
  for (int i = 0; i < desc.n_ops; ++i) {
    const zf_op_desc& op = desc.ops[i];
    if (op.kind != ZF_OP_NSC) continue;  // Roll: index map; ShiftBounds (first op): above
    // spline: g (d / d state i) -> g_next (d / d state i + 1, transformed columns), gP
    rc = spline_inv_bwd_launch(sp[i + 1], sp[i], t->nsc[i].P, g, t->d_ce, t->d_sm, g_next, t->nsc[i].gP, B, D, D / 2,
                               op.knots, t->rots[i], st);
    if (rc) return rc;
    if ((rc = nsc_reverse_mlp(t, i, B, Bg, &wq, st))) return rc;
    if ((rc = bn_param_grads(t, i, lbn, B, st))) return rc;
    if ((rc = bn_eval_reverse(t, i, t->d_sm, g_next, gc, gc_assign, B, st))) return rc;
    gc_assign = 0;
    std::swap(g, g_next);
  }
  if ((rc = wgrad_flush(wq, st))) return rc;
  if ((rc = gc_zero_unassigned(t, gc, gc_assign, B, st))) return rc;
  if (gz && (rc = sample_gz_out_launch(g, glq ? t->d_gl : nullptr, t->d_sm, gz, B, D, t->rots[desc.n_ops], st))) return rc;
  return close_gradient(t, G, false, st);
}

// ---- The whole passes ----

// Train-mode forward + loss + reverse pass from the staged batch of B rows
// (this rank's shard of a global batch of Bg rows); the loss lands in
// loss_slot(t), the gradient in G (natural blob layout, fp32).
// step_in_cast (one device, an (n)adamw update follows): the gradient cast also
// advances the optimiser's step counter, and trainer_update skips step_kernel.
// a.gc (this rank's (B, C) rows, or NULL): also d loss / d c, the condition
// columns of every coupling's d loss / d U (train.py:64-86 differentiated
// with respect to the conditions, as jax.grad(loss_fn_2) of
// examples/deep_set.ipynb does through DeepSetFlow's c = phi(x)).  It only
// adds stores: loss, G and the stepped blob keep their bits.
// a.w != NULL: the loss is -sum_b w_b lp_b / sum_b w_b with the staged weights
// d_w (the user's loss around flow.apply(..., train=True) for weighted
// samples).  The weights enter at the loss only: the forward pass and its
// batch statistics are the unweighted ones, and the reverse pass is seeded
// with the per-row cotangent d_ce in place of the constant gl.
int trainer_body(zf_trainer_t* t, const BatchArgs& a, float* G, bool step_in_cast) {
  const int D = t->D, W = t->comm.world, B = (int)a.rows;
  const long long Bg = a.global_rows;
  hipStream_t st = a.stream;
  const bool weighted = a.w != nullptr;
  const zf_flow_desc& desc = t->desc;
  auto state = [&](int i) { return t->sp[i]; };
  int rc;
  if ((rc = trainer_forward_train(t, B, Bg, a.update_stats, st))) return rc;
  const int rot = t->rots[desc.n_ops];
  // ---- latent + loss ----
  const LatentConsts lc(desc);
  float* g = t->d_g0;  // d loss / d latent: where trainer_reverse starts
  {
    const Leaves ll = leaves_for(B, Bg, W, kLeafCap);
    // leaves that tile the 256-row blocks are summed inside the loss kernel
    const bool fused = ll.rows > 0 && ll.rows <= 256 && 256 % ll.rows == 0;
    if (weighted) {
      // the sum of the weights over the loss's own leaf tree, then the rows' terms and cotangents
      hipLaunchKernelGGL(leaf_sum_f32_kernel, dim3(blocks_for(ll.n, 64)), dim3(64), 0, st, (const float*)t->d_w, B,
                         ll.rows, ll.n, t->d_leaf);
      ZF_CHECK_LAUNCH("leaf_sum_f32_kernel");
      if ((rc = launch_tree_cols(t->d_leaf, ll.n, 1, wsum_slot(t), st, t->d_leaf2))) return rc;
      if ((rc = dp_combine(t, wsum_slot(t), 1, st))) return rc;
      hipLaunchKernelGGL(zf::latent_loss_weighted_kernel, dim3(zf::blocks_for(B)), dim3(256), 0, st,
                         state(desc.n_ops), t->d_ld, (const float*)t->d_w, (const double*)wsum_slot(t), B, D, rot,
                         lc.lt, lc.a, lc.betac, lc.tnm, g, t->d_ce, t->d_rowloss, fused ? ll.rows : 0, ll.n,
                         t->d_leaf);
      ZF_CHECK_LAUNCH("latent_loss_weighted_kernel");
    } else {
      hipLaunchKernelGGL(zf::latent_loss_kernel, dim3(zf::blocks_for(B)), dim3(256), 0, st, state(desc.n_ops),
                         t->d_ld, B, Bg, D, rot, lc.lt, lc.a, lc.betac, lc.tnm, g, t->d_rowloss, fused ? ll.rows : 0,
                         ll.n, t->d_leaf);
      ZF_CHECK_LAUNCH("latent_loss_kernel");
    }
    if (!fused) {
      hipLaunchKernelGGL(leaf_sum_kernel, dim3(blocks_for(ll.n, 64)), dim3(64), 0, st, t->d_rowloss, B, ll.rows,
                         ll.n, t->d_leaf);
      ZF_CHECK_LAUNCH("leaf_sum_kernel");
    }
    if ((rc = launch_tree_cols(t->d_leaf, ll.n, 1, loss_slot(t), st, t->d_leaf2))) return rc;
    if ((rc = dp_combine(t, loss_slot(t), 1, st))) return rc;
  }
  return trainer_reverse(t, B, Bg, {weighted, false, a.gc, G, step_in_cast}, st);
}

// Eval-mode forward with stored activations and the reverse pass for one
// chunk of B <= bmax rows (zf_trainer_log_prob_vjp): the trainer's GEMMs and
// spline kernels, none of its batch reductions, weight-gradient GEMMs, fp64
// accumulators or optimiser.  The GEMM forms follow the chunk's row count
// (never the other rows' values): a row's bits depend on its own inputs and
// on how many rows share the chunk only.
int trainer_vjp_chunk(zf_trainer_t* t, const float* x, const float* c_in, const float* cot, float* lp_out, float* gx,
                      float* gc, int B, hipStream_t st) {
  int rc = trainer_stage(t, x, c_in, nullptr, B, st);  // checked by zf_trainer_log_prob_vjp
  if (rc) return rc;
  const int D = t->D;
  const zf_flow_desc& desc = t->desc;
  if ((rc = trainer_forward_eval(t, B, B, false, st))) return rc;
  // ---- latent, log_prob, the per-row cotangent ----
  float* g = t->d_g0;
  float* g_prev = t->d_g1;
  if ((rc = latent_vjp_launch(t, B, cot, lp_out, g, st))) return rc;
  if (!gx && !gc) return ZF_OK;
  // ---- reverse ----
  int gc_assign = 1;
  for (int i = desc.n_ops - 1; i >= 0; --i) {
    if (desc.ops[i].kind != ZF_OP_NSC) continue;  // Roll: index map; ShiftBounds (first op): below
    if ((rc = spline_reverse(t, i, g, g_prev, t->d_ce, 0.f, B, st))) return rc;
    if ((rc = nsc_reverse_mlp(t, i, B, B, nullptr, st))) return rc;
    if ((rc = bn_eval_reverse(t, i, t->d_ce, g_prev, gc, gc_assign, B, st))) return rc;
    gc_assign = 0;
    std::swap(g, g_prev);
  }
  if ((rc = gc_zero_unassigned(t, gc, gc_assign, B, st))) return rc;
  if (gx) {
    hipLaunchKernelGGL(sb_eval_bwd_kernel, dim3(blocks_for((int64_t)B * D)), dim3(256), 0, st,
                       (const float*)t->d_state, (const float*)g, (const float*)t->d_ce,
                       t->sb_first ? (const float*)(t->d_nat + desc.ops[0].off_sb) : nullptr, gx, B, D);
    ZF_CHECK_LAUNCH("sb_eval_bwd_kernel");
  }
  return ZF_OK;
}

// ---- The optimiser update, the captured step and the loss_grad / step entries ----

// The chain's step (zf_optim.hip): the gradient is in t->d_grad, its cast did
// not step (trainer_body without step_in_cast).
int chain_update(zf_trainer_t* t, hipStream_t st) {
  return optim_chain_step(t->d_nat, t->d_grad, t->d_mask, t->d_dmask, (long long)t->nat_floats, t->cargs,
                          t->chain_form, t->chain_clip, t->max_norm, t->chain_lr, t->sched, t->chain_adam,
                          t->chain_b1, t->chain_b2, t->d_osc, t->d_nleaf, t->n_nleaf, st);
}

int trainer_update(zf_trainer_t* t, hipStream_t st, bool step_done = false) {
  if (t->chain_on) return chain_update(t, st);
  const zf_optim_desc& o = t->opt;
  if (!step_done) {
    hipLaunchKernelGGL(step_kernel, dim3(1), dim3(1), 0, st, t->d_bc, o.b1, o.b2);
    ZF_CHECK_LAUNCH("step_kernel");
  }
  hipLaunchKernelGGL(adam_kernel, dim3(blocks_for(t->nat_floats)), dim3(256), 0, st, t->d_nat, t->d_grad, t->d_m,
                     t->d_v, t->d_mask, (long long)t->nat_floats, o.learning_rate, o.b1, o.b2, o.eps, o.weight_decay,
                     o.nesterov, t->d_bc);
  ZF_CHECK_LAUNCH("adam_kernel");
  return ZF_OK;
}

// The whole step (body + optimiser) captured once per batch size; the
// weighted step has a cache of its own, bounded the same way (weighted and
// unweighted steps may alternate on one trainer).  One device, no gc: the
// graph reads only the trainer's own buffers, which the batch is staged into.
int step_graph(zf_trainer_t* t, const BatchArgs& a, hipGraphExec_t* out) {
  std::map<int64_t, hipGraphExec_t>& graphs = a.w ? t->graphs_w : t->graphs;
  auto it = graphs.find(a.rows);
  if (it != graphs.end()) {
    *out = it->second;
    return ZF_OK;
  }
  if (graphs.size() >= 8) {  // bound the cache (batch sizes rarely vary)
    ZF_TRY_HIP(hipStreamSynchronize(t->cap));
    ZF_TRY_HIP(hipDeviceSynchronize());
    drop_graphs(graphs);
  }
  ZF_TRY_HIP(hipStreamBeginCapture(t->cap, hipStreamCaptureModeThreadLocal));
  BatchArgs b = a;
  b.gc = nullptr;
  b.stream = t->cap;
  int rc = trainer_body(t, b, t->d_grad, !t->chain_on);
  if (!rc) rc = trainer_update(t, t->cap, !t->chain_on);
  hipGraph_t g = nullptr;
  const hipError_t e = hipStreamEndCapture(t->cap, &g);
  if (!rc && e != hipSuccess) rc = hip_status(e, "hipStreamEndCapture");
  hipGraphExec_t exec = nullptr;
  if (!rc) {
    const hipError_t ei = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
    if (ei != hipSuccess) rc = hip_status(ei, "hipGraphInstantiate");
  }
  if (g) (void)hipGraphDestroy(g);
  if (rc) return rc;
  graphs[a.rows] = exec;
  *out = exec;
  return ZF_OK;
}

inline int copy_loss(zf_trainer_t* t, const BatchArgs& a) {
  if (a.loss) ZF_TRY_HIP(hipMemcpyAsync(a.loss, loss_slot(t), sizeof(double), hipMemcpyDeviceToDevice, a.stream));
  return ZF_OK;
}

// Every zf_trainer_loss_grad* entry: the loss and its gradient (and gc).
int run_loss_grad(zf_trainer_t* t, const BatchArgs& a) {
  set_pending(t, kPendNone);  // the arena is about to be overwritten
  int rc = check_batch(t, a);
  if (!rc) rc = trainer_stage(t, a.x, a.c, a.w, a.rows, a.stream);
  if (!rc) rc = trainer_body(t, a, a.grad ? a.grad : t->d_grad, false);
  return rc ? rc : copy_loss(t, a);
}

// Every zf_trainer_step* entry (update_stats = 1, the gradient in d_grad).
// The captured graph writes no gc and holds no collective: a step with gc,
// or with a communicator, launches the same kernels in the same order
// eagerly, so the same bits (tests/test_gpu_train.py::test_step_graph_matches_eager).
int run_step(zf_trainer_t* t, const BatchArgs& a) {
  set_pending(t, kPendNone);
  int rc = check_batch(t, a);
  if (!rc) rc = trainer_stage(t, a.x, a.c, a.w, a.rows, a.stream);
  if (rc) return rc;
  const bool one_device = t->comm.world == 1;
  if (!(t->C > 0 && a.gc) && t->use_graph && one_device) {
    hipGraphExec_t exec = nullptr;
    if ((rc = step_graph(t, a, &exec))) return rc;
    ZF_TRY_HIP(hipGraphLaunch(exec, a.stream));
  } else {
    const bool step_in_cast = !t->chain_on && one_device;
    rc = trainer_body(t, a, t->d_grad, step_in_cast);
    if (!rc) rc = trainer_update(t, a.stream, step_in_cast);
    if (rc) return rc;
  }
  t->t += 1;
  return copy_loss(t, a);
}

// ZF_EINVAL while a ShiftBounds dim that maps through the stored xmin / xmax
// still holds the initial +-inf (no train-mode pass has run): its inverse is
// undefined.  Read back once; training only widens finite bounds.
int check_sample_bounds(zf_trainer_t* t, hipStream_t st) {
  if (t->sb_ok || !t->sb_first) return ZF_OK;
  std::vector<float> rows((size_t)8 * t->D);
  ZF_TRY_HIP(hipStreamSynchronize(st));
  ZF_TRY_HIP(hipMemcpy(rows.data(), t->d_nat + t->desc.ops[0].off_sb, rows.size() * sizeof(float), hipMemcpyDeviceToHost));
  for (int j = 0; j < t->D; ++j) {
    if ((int)rows[8 * j] == ZF_SB_BOTH) continue;
    if (!std::isfinite(rows[8 * j + 3]) || !std::isfinite(rows[8 * j + 4]))
      return einval("ShiftBounds: the stored bounds of dim %d are still the initial +-inf (no train-mode pass has set "
                    "them): the inverse is undefined", j);
  }
  t->sb_ok = true;
  return ZF_OK;
}

}  // namespace
}  // namespace zf

extern "C" {

// The eight loss_grad / step entries are views of run_loss_grad / run_step:
// w == NULL is the unweighted loss, gc == NULL (or C == 0) writes no gc, and
// the plain entries' global batch is B rows on every rank.
int zf_trainer_loss_grad_weighted_shard(zf_trainer_t* t, const float* x, const float* c, const float* w, int64_t rows,
                                        int64_t global_rows, int update_stats, double* loss, float* grad, float* gc,
                                        void* stream) {
  if (!t) return zf::einval("trainer is NULL");
  return zf::run_loss_grad(t, {x, c, w, rows, global_rows, update_stats, loss, grad, gc, (hipStream_t)stream});
}

int zf_trainer_loss_grad_cond_shard(zf_trainer_t* t, const float* x, const float* c, int64_t rows,
                                    int64_t global_rows, int update_stats, double* loss, float* grad, float* gc,
                                    void* stream) {
  if (!t) return zf::einval("trainer is NULL");
  return zf::run_loss_grad(t, {x, c, nullptr, rows, global_rows, update_stats, loss, grad, gc, (hipStream_t)stream});
}

int zf_trainer_loss_grad_shard(zf_trainer_t* t, const float* x, const float* c, int64_t rows, int64_t global_rows,
                               int update_stats, double* loss, float* grad, void* stream) {
  if (!t) return zf::einval("trainer is NULL");
  return zf::run_loss_grad(
      t, {x, c, nullptr, rows, global_rows, update_stats, loss, grad, nullptr, (hipStream_t)stream});
}

int zf_trainer_loss_grad(zf_trainer_t* t, const float* x, const float* c, int64_t B, int update_stats,
                         double* loss, float* grad, void* stream) {
  if (!t) return zf::einval("trainer is NULL");
  return zf::run_loss_grad(
      t, {x, c, nullptr, B, B * t->comm.world, update_stats, loss, grad, nullptr, (hipStream_t)stream});
}

int zf_trainer_step_weighted_shard(zf_trainer_t* t, const float* x, const float* c, const float* w, int64_t rows,
                                   int64_t global_rows, double* loss, float* gc, void* stream) {
  if (!t) return zf::einval("trainer is NULL");
  return zf::run_step(t, {x, c, w, rows, global_rows, 1, loss, nullptr, gc, (hipStream_t)stream});
}

int zf_trainer_step_cond_shard(zf_trainer_t* t, const float* x, const float* c, int64_t rows, int64_t global_rows,
                               double* loss, float* gc, void* stream) {
  if (!t) return zf::einval("trainer is NULL");
  return zf::run_step(t, {x, c, nullptr, rows, global_rows, 1, loss, nullptr, gc, (hipStream_t)stream});
}

int zf_trainer_step_shard(zf_trainer_t* t, const float* x, const float* c, int64_t rows, int64_t global_rows,
                          double* loss, void* stream) {
  if (!t) return zf::einval("trainer is NULL");
  return zf::run_step(t, {x, c, nullptr, rows, global_rows, 1, loss, nullptr, nullptr, (hipStream_t)stream});
}

int zf_trainer_step(zf_trainer_t* t, const float* x, const float* c, int64_t B, double* loss, void* stream) {
  if (!t) return zf::einval("trainer is NULL");
  return zf::run_step(t, {x, c, nullptr, B, B * t->comm.world, 1, loss, nullptr, nullptr, (hipStream_t)stream});
}

int zf_trainer_log_prob_vjp(zf_trainer_t* t, const float* x, const float* c, const float* cot, float* log_prob,
                            float* gx, float* gc, int64_t N, void* stream) {
  if (!t) return zf::einval("trainer is NULL");
  zf::set_pending(t, zf::kPendNone);
  hipStream_t st = (hipStream_t)stream;
  const int rc0 = zf::check_batch(t, {x, c, nullptr, N, N, 0, nullptr, nullptr, nullptr, st}, zf::kBatchChunked);
  if (rc0) return rc0;
  if (t->desc.latent == ZF_LATENT_NONE) return zf::einval("flow has no latent distribution");
  const int D = t->D, C = t->C;
  for (int64_t off = 0; off < N; off += t->bmax) {
    const int B = (int)std::min<int64_t>(t->bmax, N - off);
    const int rc = zf::trainer_vjp_chunk(t, x + off * D, C > 0 ? c + off * C : nullptr, cot ? cot + off : nullptr,
                                         log_prob ? log_prob + off : nullptr, gx ? gx + off * D : nullptr,
                                         gc && C > 0 ? gc + off * C : nullptr, B, st);
    if (rc) return rc;
  }
  return ZF_OK;
}

// ---- custom losses: forward, backward(cotangent), apply_gradient ----
// The user's loss around flow.apply (train.py:64-86, flow.py:22-48) is host
// code between two calls: forward hands out the per-row log_prob, backward
// takes d loss / d log_prob per row and returns the parameter gradient.
int zf_trainer_forward(zf_trainer_t* t, const float* x, const float* c, int64_t rows, int64_t global_rows, int train,
                       int update_stats, float* log_prob, void* stream) {
  if (!t) return zf::einval("trainer is NULL");
  zf::set_pending(t, zf::kPendNone);
  hipStream_t st = (hipStream_t)stream;
  const int rc0 = zf::check_batch(t, {x, c, nullptr, rows, global_rows, update_stats, nullptr, nullptr, nullptr, st});
  if (rc0) return rc0;
  if (!log_prob) return zf::einval("log_prob is NULL");
  if (!train && update_stats) return zf::einval("update_stats needs train mode (eval mode reads the stored statistics)");
  if (t->desc.latent == ZF_LATENT_NONE) return zf::einval("flow has no latent distribution");
  const int B = (int)rows;
  int rc = zf::trainer_stage(t, x, c, nullptr, rows, st);
  if (!rc)
    rc = train ? zf::trainer_forward_train(t, B, global_rows, update_stats, st)
               : zf::trainer_forward_eval(t, B, global_rows, true, st);
  if (rc) return rc;
  // log_prob with nan_to_num; its ce / gz outputs are rewritten by backward's launch
  if ((rc = zf::latent_vjp_launch(t, B, nullptr, log_prob, t->d_g0, st))) return rc;
  zf::set_pending(t, train ? zf::kPendTrain : zf::kPendEval, rows, global_rows);
  return ZF_OK;
}

int zf_trainer_backward(zf_trainer_t* t, const float* cot, float* grad, float* gc, void* stream) {
  if (!t) return zf::einval("trainer is NULL");
  if (t->pend_mode != zf::kPendTrain && t->pend_mode != zf::kPendEval)  // a sampling pass is not a forward
    return zf::einval("no forward pending");
  const bool eval = t->pend_mode == zf::kPendEval;
  const int B = (int)t->pend_rows;
  const long long Bg = t->pend_global;
  zf::set_pending(t, zf::kPendNone);  // one backward per forward
  hipStream_t st = (hipStream_t)stream;
  // ce = cot where log_prob is finite before nan_to_num (0 elsewhere), gz = ce . d latent_lp / dz
  const int rc = zf::latent_vjp_launch(t, B, cot, nullptr, t->d_g0, st);
  if (rc) return rc;
  return zf::trainer_reverse(t, B, Bg, {true, eval, gc, grad ? grad : t->d_grad, false}, st);
}

int zf_trainer_apply_gradient(zf_trainer_t* t, const float* grad, void* stream) {
  if (!t) return zf::einval("trainer is NULL");
  zf::set_pending(t, zf::kPendNone);
  hipStream_t st = (hipStream_t)stream;
  if (grad && grad != t->d_grad)
    ZF_TRY_HIP(hipMemcpyAsync(t->d_grad, grad, (size_t)t->nat_floats * sizeof(float), hipMemcpyDeviceToDevice, st));
  const int rc = zf::trainer_update(t, st);
  if (rc) return rc;
  t->t += 1;
  return ZF_OK;
}

// ---- gradients through sampling: sample_forward, sample_backward ----
int zf_trainer_sample_forward(zf_trainer_t* t, const float* z, const float* c, int64_t rows, int64_t global_rows,
                              float* x, float* log_q, void* stream) {
  if (!t) return zf::einval("trainer is NULL");
  zf::set_pending(t, zf::kPendNone);
  hipStream_t st = (hipStream_t)stream;
  int rc = zf::check_batch(t, {z, c, nullptr, rows, global_rows, 0, nullptr, nullptr, nullptr, st}, zf::kBatchSample);
  if (rc) return rc;
  if (!x) return zf::einval("x is NULL");
  if (t->desc.latent == ZF_LATENT_NONE) return zf::einval("flow has no latent distribution");
  if ((rc = zf::check_sample_bounds(t, st))) return rc;
  const int B = (int)rows;
  if (t->C > 0)
    ZF_TRY_HIP(hipMemcpyAsync(t->d_c, c, (size_t)rows * t->C * sizeof(float), hipMemcpyDeviceToDevice, st));
  if ((rc = zf::sample_rot_in_launch(z, t->sp[t->n_ops], B, t->D, t->rots[t->n_ops], st))) return rc;
  if ((rc = zf::trainer_sample_forward(t, B, global_rows, x, log_q, st))) return rc;
  zf::set_pending(t, zf::kPendSample, rows, global_rows);
  return ZF_OK;
}

int zf_trainer_sample_backward(zf_trainer_t* t, const float* gx, const float* glq, float* grad, float* gz, float* gc,
                               void* stream) {
  if (!t) return zf::einval("trainer is NULL");
  if (t->pend_mode != zf::kPendSample) return zf::einval("no forward pending");
  if (!gx) return zf::einval("gx is NULL");
  const int B = (int)t->pend_rows;
  const long long Bg = t->pend_global;
  zf::set_pending(t, zf::kPendNone);  // one backward per forward
  return zf::trainer_sample_reverse(t, B, Bg, gx, glq, grad ? grad : t->d_grad, gz, gc, (hipStream_t)stream);
}

int zf_trainer_get_blob(zf_trainer_t* t, float* blob_host) {
  if (!t || !blob_host) return zf::einval("NULL argument");
  ZF_TRY_HIP(hipDeviceSynchronize());
  ZF_TRY_HIP(hipMemcpy(blob_host, t->d_nat, t->nat_floats * sizeof(float), hipMemcpyDeviceToHost));
  return ZF_OK;
}

int zf_trainer_set_blob(zf_trainer_t* t, const float* blob_host) {
  if (!t || !blob_host) return zf::einval("NULL argument");
  zf::set_pending(t, zf::kPendNone);
  t->sb_ok = false;
  ZF_TRY_HIP(hipDeviceSynchronize());
  ZF_TRY_HIP(hipMemcpy(t->d_nat, blob_host, t->nat_floats * sizeof(float), hipMemcpyHostToDevice));
  return ZF_OK;
}

}  // extern "C"

namespace zf {
namespace {

void free_chain(zf_trainer_t* t) {
  for (void* p : t->opt_bufs) (void)hipFree(p);
  t->opt_bufs.clear();
  t->d_dmask = nullptr;
  t->d_nleaf = nullptr;
  t->d_osc = nullptr;
  t->n_slots = 0;
  t->chain_on = false;
}

int opt_alloc(zf_trainer_t* t, void** p, size_t bytes) {
  *p = nullptr;
  ZF_TRY_HIP(hipMalloc(p, bytes ? bytes : 1));
  t->opt_bufs.push_back(*p);
  ZF_TRY_HIP(hipMemset(*p, 0, bytes ? bytes : 1));
  return ZF_OK;
}

}  // namespace
}  // namespace zf

extern "C" {

int zf_trainer_set_optim_chain(zf_trainer_t* t, const zf_optim_chain* chain, const unsigned char* decay_mask) {
  if (!t || !chain) return zf::einval("NULL argument");
  zf::set_pending(t, zf::kPendNone);
  // the stage list, its form and what the prologue needs (zf_optim.hip)
  zf::ChainPlan plan;
  int rc = zf::optim_plan_chain(chain, decay_mask != nullptr, &plan);
  if (rc) return rc;
  zf::ChainArgs a = plan.args;
  const int slots = plan.n_slots;
  ZF_TRY_HIP(hipStreamSynchronize(t->cap));
  ZF_TRY_HIP(hipDeviceSynchronize());
  zf::drop_graphs(t->graphs);
  zf::drop_graphs(t->graphs_w);
  zf::free_chain(t);
  const size_t need = (size_t)t->nat_floats;
  for (int k = 0; k < slots && !rc; ++k) rc = zf::opt_alloc(t, (void**)&a.slot[k], need * sizeof(float));
  if (!rc && plan.masked) {
    rc = zf::opt_alloc(t, (void**)&t->d_dmask, need);
    if (!rc) {
      const hipError_t e = hipMemcpy(t->d_dmask, decay_mask, need, hipMemcpyHostToDevice);
      if (e != hipSuccess) rc = zf::hip_status(e, "zf_trainer_set_optim_chain mask");
    }
  }
  t->n_nleaf = (int)((t->nat_floats + zf::kNormSpan - 1) / zf::kNormSpan);
  if (!rc) rc = zf::opt_alloc(t, (void**)&t->d_nleaf, (size_t)(t->n_nleaf > 0 ? t->n_nleaf : 1) * sizeof(double));
  if (!rc) rc = zf::opt_alloc(t, (void**)&t->d_osc, sizeof(zf::OptScalars));
  if (rc) {
    zf::free_chain(t);
    return rc;
  }
  t->cargs = a;
  t->chain_form = plan.form;
  t->n_slots = slots;
  t->chain_clip = plan.clip;
  t->max_norm = plan.max_norm;
  t->chain_lr = plan.has_lr;
  if (plan.has_lr) t->sched = plan.sched;
  t->chain_adam = plan.has_adam;
  t->chain_b1 = plan.b1;
  t->chain_b2 = plan.b2;
  t->t = 0;
  t->chain_on = true;
  return ZF_OK;
}

static int opt_slot_ptr(zf_trainer_t* t, int slot, float** p) {
  if (!t) return zf::einval("trainer is NULL");
  const int n = t->chain_on ? t->n_slots : 2;
  if (slot < 0 || slot >= n) return zf::einval("optimiser slot %d outside [0, %d)", slot, n);
  *p = t->chain_on ? t->cargs.slot[slot] : (slot == 0 ? t->d_m : t->d_v);
  return ZF_OK;
}

int zf_trainer_get_opt_slot(zf_trainer_t* t, int slot, float* host_floats) {
  float* p = nullptr;
  const int rc = opt_slot_ptr(t, slot, &p);
  if (rc) return rc;
  if (!host_floats) return zf::einval("NULL argument");
  ZF_TRY_HIP(hipDeviceSynchronize());
  ZF_TRY_HIP(hipMemcpy(host_floats, p, t->nat_floats * sizeof(float), hipMemcpyDeviceToHost));
  return ZF_OK;
}

int zf_trainer_set_opt_slot(zf_trainer_t* t, int slot, const float* host_floats) {
  float* p = nullptr;
  const int rc = opt_slot_ptr(t, slot, &p);
  if (rc) return rc;
  if (!host_floats) return zf::einval("NULL argument");
  ZF_TRY_HIP(hipDeviceSynchronize());
  ZF_TRY_HIP(hipMemcpy(p, host_floats, t->nat_floats * sizeof(float), hipMemcpyHostToDevice));
  return ZF_OK;
}

int zf_trainer_get_opt_scalars(zf_trainer_t* t, int64_t* count, double* learning_rate, double* grad_norm) {
  if (!t) return zf::einval("trainer is NULL");
  ZF_TRY_HIP(hipDeviceSynchronize());
  if (t->chain_on) {
    zf::OptScalars sc;
    ZF_TRY_HIP(hipMemcpy(&sc, t->d_osc, sizeof(sc), hipMemcpyDeviceToHost));
    if (count) *count = sc.count;
    if (learning_rate) *learning_rate = (double)sc.lr;
    if (grad_norm) *grad_norm = sc.count > 0 ? sc.norm : (double)__builtin_nanf("");
    if (learning_rate && sc.count == 0) *learning_rate = (double)__builtin_nanf("");  // no step yet
    return ZF_OK;
  }
  int c = 0;
  ZF_TRY_HIP(hipMemcpy(&c, t->d_bc, sizeof(int), hipMemcpyDeviceToHost));
  if (count) *count = c;
  if (learning_rate) *learning_rate = (double)t->opt.learning_rate;
  if (grad_norm) *grad_norm = (double)__builtin_nanf("");
  return ZF_OK;
}

int zf_trainer_set_opt_count(zf_trainer_t* t, int64_t count) {
  if (!t) return zf::einval("trainer is NULL");
  if (count < 0 || count > 0x7fffffff) return zf::einval("optimiser count %lld outside [0, 2^31)", (long long)count);
  ZF_TRY_HIP(hipDeviceSynchronize());
  if (t->chain_on) {
    const long long c = count;
    ZF_TRY_HIP(hipMemcpy(&t->d_osc->count, &c, sizeof(c), hipMemcpyHostToDevice));
  } else {
    const int rc = zf::optim_set_count(t->d_bc, (int)count, t->opt.b1, t->opt.b2);
    if (rc) return rc;
    ZF_TRY_HIP(hipDeviceSynchronize());
  }
  t->t = count;
  return ZF_OK;
}

}  // extern "C"

// ---- Entry points of the layered eval path (zf_layered.hip) -----------------
namespace zf {

int dense_gemm(long long Mg, int M, int N, int K, const float* A, int lda, const float* W, int ldw, float* C,
               int ldc, float* H, hipStream_t st, const float* bias, int act, unsigned* rmax) {
  if (rmax && M > 0) ZF_TRY_HIP(hipMemsetAsync(rmax, 0, (size_t)M * sizeof(unsigned), st));
  bool done = false;
  const int rc = gemm(false, Mg, M, N, K, A, lda, W, ldw, C, ldc, st, bias ? kEpiBias : kEpiNone, bias, H, nullptr,
                      act, nullptr, 0, rmax, &done);
  if (rc || !rmax || done || M <= 0) return rc;
  hipLaunchKernelGGL(row_absmax_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, M, N, H ? H : C, ldc, rmax);
  ZF_CHECK_LAUNCH("row_absmax_kernel");
  return ZF_OK;
}

int spline_rows(bool inverse, const float* s_in, float* s_out, const float* P, float* ld, int B, int D, int dt,
                int K, int rot, hipStream_t st) {
  return spline_rows_launch(inverse, s_in, s_out, P, ld, B, D, dt, K, rot, st);
}

}  // namespace zf
