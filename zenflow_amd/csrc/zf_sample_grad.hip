// Device code of the gradients through sampling (zf_train_sample.h) and its
// host launchers, which zf_train.hip's drivers (trainer_sample_forward,
// trainer_sample_reverse) call.  A translation unit of its own, as
// zf_optim.hip is: zf_train.hip gains host code only, so the code object of
// the trainer's kernels keeps its bytes and its timing (Training).
#include "zf_train_sample.h"

namespace zf {

int spline_inv_ld_launch(const float* s_in, float* s_out, const float* P, float* ld, float* dead, int B, int D, int dt,
                         int K, int rot, hipStream_t st) {
  if (B <= 0) return ZF_OK;
  if (dt < 1 || dt > kSplThreads || K < 1 || K > kMaxK) return enotsup("sample gradient: transformed dims or knots out of range");
  const int rpb = kSplThreads / dt;
  const size_t lds = (size_t)kSplThreads * (3 * K - 1) * sizeof(float);
#define ZF_SPL(KTV)                                                                                             \
  hipLaunchKernelGGL((spline_inv_ld_kernel<KTV>), dim3(blocks_for(B, rpb)), dim3(kSplThreads), lds, st, s_in, \
                     s_out, P, ld, dead, B, D, dt, K, rot)
  ZF_KNOT_DISPATCH(K, ZF_SPL);
#undef ZF_SPL
  ZF_CHECK_LAUNCH("spline_inv_ld_kernel");
  return ZF_OK;
}

int spline_inv_bwd_launch(const float* s_y, const float* s_x, const float* P, const float* g_out, const float* glr,
                          const float* mask, float* g_in, float* gP, int B, int D, int dt, int K, int rot,
                          hipStream_t st) {
  if (B <= 0) return ZF_OK;
  if (dt < 1 || dt > kSplThreads || K < 1 || K > kMaxK) return enotsup("sample gradient: transformed dims or knots out of range");
  const int rpb = kSplThreads / dt;
  const size_t lds = (size_t)kSplThreads * (3 * K - 1) * sizeof(float);
#define ZF_SPL(KTV)                                                                                            \
  hipLaunchKernelGGL((spline_inv_bwd_kernel<KTV>), dim3(blocks_for(B, rpb)), dim3(kSplThreads), lds, st, s_y, \
                     s_x, P, g_out, glr, mask, g_in, gP, B, D, dt, K, rot)
  ZF_KNOT_DISPATCH(K, ZF_SPL);
#undef ZF_SPL
  ZF_CHECK_LAUNCH("spline_inv_bwd_kernel");
  return ZF_OK;
}

int sb_eval_inv_launch(const float* s1, float* s0, float* x, const float* sb, float* ld, const float* lat,
                       const float* fin, float* mask, float* log_q, int B, int D, hipStream_t st) {
  hipLaunchKernelGGL(sb_eval_inv_kernel, dim3(blocks_for(B)), dim3(256), 0, st, s1, s0, x, sb, ld, lat, fin, mask,
                     log_q, B, D);
  ZF_CHECK_LAUNCH("sb_eval_inv_kernel");
  return ZF_OK;
}

int sb_eval_inv_bwd_launch(const float* s1, const float* gx, const float* ce, const float* mask, const float* sb,
                           float* g, int B, int D, hipStream_t st) {
  hipLaunchKernelGGL(sb_eval_inv_bwd_kernel, dim3(blocks_for((long long)B * D)), dim3(256), 0, st, s1, gx, ce, mask,
                     sb, g, B, D);
  ZF_CHECK_LAUNCH("sb_eval_inv_bwd_kernel");
  return ZF_OK;
}

int sample_rot_in_launch(const float* z, float* s, int B, int D, int rot, hipStream_t st) {
  hipLaunchKernelGGL(rot_in_kernel, dim3(blocks_for((long long)B * D)), dim3(256), 0, st, z, s, B, D, rot);
  ZF_CHECK_LAUNCH("rot_in_kernel");
  return ZF_OK;
}

int sample_mask_cot_launch(const float* glq, const float* mask, float* ce, int B, hipStream_t st) {
  hipLaunchKernelGGL(mask_cot_kernel, dim3(blocks_for(B)), dim3(256), 0, st, glq, mask, ce, B);
  ZF_CHECK_LAUNCH("mask_cot_kernel");
  return ZF_OK;
}

int sample_gz_out_launch(const float* g, const float* gl, const float* mask, float* gz, int B, int D, int rot,
                         hipStream_t st) {
  hipLaunchKernelGGL(gz_out_kernel, dim3(blocks_for((long long)B * D)), dim3(256), 0, st, g, gl, mask, gz, B, D, rot);
  ZF_CHECK_LAUNCH("gz_out_kernel");
  return ZF_OK;
}

}  // namespace zf
