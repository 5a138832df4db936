// Optimiser chains (include/zenflow_amd.h, ZF_OPT_*): what the trainer
// (zf_train.hip) and the chain kernels' translation unit (zf_optim.hip) share.
#pragma once
#include "zf_internal.h"

namespace zf {

// The device scalars of a chain (zf_trainer_get_opt_scalars reads them back).
struct OptScalars {
  long long count;  // updates applied so far
  double norm;      // the last step's gradient norm (NaN without the clip)
  float lr, clip, bc1, bc1n, bc2, _pad;
};

constexpr int kNormSpan = 4096;  // blob entries per leaf of the gradient's sum of squares

// The stage list as the update kernel takes it (a kernel argument).
struct ChainStage {
  int kind, flags, slot;  // slot: the stage's first moment array
  float p[4];
};
struct ChainArgs {
  int n;
  ChainStage st[ZF_OPT_MAX_STAGES];
  float* slot[ZF_OPT_MAX_SLOTS];
};

constexpr int kFormGeneric = 0;  // any valid chain: a loop over the stages
constexpr int kFormSgd = 1;      // [clip_by_global_norm] [trace] scale_by_learning_rate
constexpr int kFormAdam = 2;     // [clip_by_global_norm] scale_by_adam [add_decayed_weights] scale_by_learning_rate
constexpr int kFormLion = 3;     // [clip_by_global_norm] scale_by_lion [add_decayed_weights] scale_by_learning_rate

// A validated zf_optim_chain as its owner (the trainer, a conditioning
// network) holds it: the stage list without its moment arrays, the form, and
// what the prologue needs.
struct ChainPlan {
  ChainArgs args{};
  int form = kFormGeneric;
  int n_slots = 0;
  bool clip = false, has_lr = false, has_adam = false, masked = false;
  float max_norm = 0.f, b1 = 0.f, b2 = 0.f;
  zf_schedule sched{};
};

// Validate `chain` (ZF_EINVAL / ZF_ENOTSUP, the message names the stage) and
// lower it to `out`.  has_decay_mask: the caller has a mask for a masked
// add_decayed_weights.  Host-side only.
int optim_plan_chain(const zf_optim_chain* chain, bool has_decay_mask, ChainPlan* out);

// One step of the chain on stream st: [sum of squares] -> prologue -> update.
// prm / g / mask: the blob, its gradient and the parameter mask (n entries);
// dmask: the decay mask or NULL; leaf: ceil(n / kNormSpan) doubles.
int optim_chain_step(float* prm, const float* g, const unsigned char* mask, const unsigned char* dmask, long long n,
                     const ChainArgs& a, int form, bool clip, float max_norm, bool has_lr, const zf_schedule& sched,
                     bool has_adam, float b1, float b2, OptScalars* sc, double* leaf, int n_leaves, hipStream_t st);

// The (n)adamw step counter bc[4] (step_update, zf_train_kernels.h) as `count` steps leave it.
int optim_set_count(float* bc, int count, float b1, float b2);

}  // namespace zf
