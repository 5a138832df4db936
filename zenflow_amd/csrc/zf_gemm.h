// The trainer's GEMM library: C[M,N] = A[M,K] . op(B) in fp32 with fused
// epilogues (bias + activation, or the activation's derivative).  gemm()
// picks one form from the GLOBAL batch's row count Mg, so every data-parallel
// shard runs the kernel, and gets the bits, of the one-device step:
//   at least 512 tiles of 128 x 128 over Mg rows (large batches):
//     K <= 8, B not transposed    gemm_small_k4_kernel, four outputs per thread (N % 4 == 0,
//                                 16-B aligned C / H rows), else gemm_small_k_kernel
//     K % 8 == 0, aligned rows    gemm_x3_kernel: bf16x3 split MFMA (ZF_TRAIN_X3=0: the next)
//     otherwise                   mgemm_kernel<128, 128>: fp32 MFMA, one accumulator set
//   fewer (small batches), all with the bits of mgemm_kernel<64, 64>'s four interleaved sets:
//     K <= 8, B not transposed    gemm_small_k_kernel, one thread per output
//     < 256 tiles, K >= 64        the four split sets + gemm_combine_kernel
//     otherwise                   mgemm_kernel<64, 64> itself
//   (the first two only when the caller gives the `split` workspace; ZF_TRAIN_SPLITQ=0: none)
// mgemm_kernel's weight-gradient (split-K) form is launched by zf_reduce.h;
// row_absmax_kernel serves the layered eval path (dense_gemm, zf_train.hip).
#pragma once
#include "zf_act.h"
#include "zf_internal.h"
#include "zf_x3_tile.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>

namespace zf {
namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));

// ---- GEMM on fp32 MFMA: C[M,N] = op(A)[M,K] . op(B)[K,N], row-major ----------
// v_mfma_f32_32x32x2_f32 is a k-ordered f32 fma chain (exact f32, the same
// numerics as a scalar fmaf loop).  Block tile BM x BN x 32 staged through LDS
// (k-major, +1 padding: the transposing stores are conflict-free), 4 waves in
// 2 x 2, each (BM/2) x (BN/2) as 32 x 32 MFMA tiles; the next k-tile's global
// loads are in flight in registers while the current one is multiplied.
// Epilogues fused into the store:
//   kEpiNone   C = acc
//   kEpiBias   z = acc + bias[n]; C = z; H = act(z) if H (flax.linen.swish, or
//              the op's other activation, zf_act.h)
//   kEpiDSwish C = acc * act'(Z[m, n])  (gradient through the activation)
// WG (weight gradients, split-K over the batch): block z multiplies rows
// [z*KC, (z+1)*KC) into part[z][M+1][N]; row M is the bias gradient, the
// column sums of the B tile (op(B) = layer-output gradient), which blocks with
// blockIdx.y == 0 form on the VALU beside the MFMAs.
constexpr int MBK = 32;
enum { kEpiNone = 0, kEpiBias = 1, kEpiDSwish = 2 };

// The fused store of one output element (both GEMM forms below).
__device__ __forceinline__ void gemm_epilogue(float v, int n, long long o, float* __restrict__ C, int epi,
                                              const float* __restrict__ bias, float* __restrict__ H,
                                              const float* __restrict__ Z, int act) {
  if (epi == kEpiBias) {
    v = v + bias[n];
    if (H) H[o] = act == ZF_ACT_SWISH ? v * sigmoidf(v) : act_other(act, v);
  } else if (epi == kEpiDSwish) {
    const float z = Z[o];
    if (act == ZF_ACT_SWISH) {
      const float sg = sigmoidf(z);
      v = v * (sg + z * sg * (1.0f - sg));
    } else {
      v = v * act_other_grad(act, z);
    }
  }
  if (C) C[o] = v;  // null: the eval path keeps only the activation H
}

// The same for four consecutive columns n..n+3 (n % 4 == 0 < N, N % 4 == 0,
// 16-B aligned rows): one dwordx4 per array instead of four dword stores.
__device__ __forceinline__ void gemm_epilogue4(float4 v, int n, long long o, float* __restrict__ C, int epi,
                                               const float* __restrict__ bias, float* __restrict__ H,
                                               const float* __restrict__ Z, int act) {
  float x[4] = {v.x, v.y, v.z, v.w};
  if (epi == kEpiBias) {
    // four scalar loads: a Dense bias inside the natural blob need not be
    // 16-B aligned (the layered path's biases alternate), and the WIDE
    // epilogue should not depend on it
    x[0] = x[0] + bias[n];
    x[1] = x[1] + bias[n + 1];
    x[2] = x[2] + bias[n + 2];
    x[3] = x[3] + bias[n + 3];
    if (H) {
      float y[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) y[t] = act == ZF_ACT_SWISH ? x[t] * sigmoidf(x[t]) : act_other(act, x[t]);
      *reinterpret_cast<float4*>(H + o) = float4{y[0], y[1], y[2], y[3]};
    }
  } else if (epi == kEpiDSwish) {
    const float4 z4 = *reinterpret_cast<const float4*>(Z + o);
    const float z[4] = {z4.x, z4.y, z4.z, z4.w};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (act == ZF_ACT_SWISH) {
        const float sg = sigmoidf(z[t]);
        x[t] = x[t] * (sg + z[t] * sg * (1.0f - sg));
      } else {
        x[t] = x[t] * act_other_grad(act, z[t]);
      }
    }
  }
  if (C) *reinterpret_cast<float4*>(C + o) = float4{x[0], x[1], x[2], x[3]};
}

// SPLITQ: block z = q of a 64 x 64 tile multiplies only the k-pairs
// p = q (mod 4) — exactly accumulator set q of the NACC = 4 kernel, in the
// same order (trailing all-zero pairs aside, which only turn -0 into +0) —
// into part[q][M][N]; gemm_combine_kernel then forms
// (P0 + P1) + (P2 + P3) and the epilogue: the same bits from four times the
// blocks (small batches: 1024 rows give 32 tiles for 256 CUs).
// The block body, with the block's coordinates passed in (mgemm_kernel: its
// blockIdx; wgrad_group_kernel: decoded from one launch over several GEMMs).
// SW: no activation but swish in the epilogue (its code only; the generic
// form's act switch made the 128 x 128 kernel ~255 KB, fetched cold at
// every epilogue)
template <int BM, int BN, bool TA, bool TB, bool WG, bool SPLITQ, bool SW = false>
__device__ __forceinline__ void mgemm_body(const uint3 bid, int M, int N, int K, const float* __restrict__ A, int lda,
                                           const float* __restrict__ B, int ldb, float* __restrict__ C, int ldc,
                                           int epi, const float* __restrict__ bias, float* __restrict__ H,
                                           const float* __restrict__ Z, int KC, int act) {
  constexpr int NA = BM * MBK / 256, NB = BN * MBK / 256;  // tile elements per thread
  constexpr int TM = BM / 64, TN = BN / 64;                // 32x32 tiles per wave
  __shared__ float As[MBK][BM + 1];
  __shared__ float Bs[MBK][BN + 1];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm0 = (wave >> 1) * (BM / 2), wn0 = (wave & 1) * (BN / 2);
  const int m0 = bid.y * BM, n0 = bid.x * BN;
  const int kbeg = WG ? bid.z * KC : 0;
  // SPLITQ: block q runs a virtual k range holding only its k-pairs
  // p = q, q + 4, q + 8, ... (virtual pair v = real pair 4 v + q), so one
  // k-tile of loads serves 16 of its pairs instead of 4
  const int q4 = SPLITQ ? (int)bid.z : 0;
  const int kend = WG ? min(K, kbeg + KC) : SPLITQ ? 2 * max(0, ((K + 1) / 2 - q4 + 3) / 4) : K;
  auto real_k = [&](int k) { return SPLITQ ? 2 * (4 * (k >> 1) + q4) + (k & 1) : k; };
  const int kmax = SPLITQ ? K : kend;
  float ra[NA], rb[NB];
  auto load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int e = tid + 256 * i;
      const int mm = TA ? (e % BM) : (e / MBK), kk = TA ? (e / BM) : (e % MBK);
      const int m = m0 + mm, k = real_k(k0 + kk);
      ra[i] = (m < M && k0 + kk < kend && k < kmax) ? (TA ? A[(long long)k * lda + m] : A[(long long)m * lda + k])
                                                    : 0.f;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int e = tid + 256 * i;
      const int nn = TB ? (e / MBK) : (e % BN), kk = TB ? (e % MBK) : (e / BN);
      const int n = n0 + nn, k = real_k(k0 + kk);
      rb[i] = (n < N && k0 + kk < kend && k < kmax) ? (TB ? B[(long long)n * ldb + k] : B[(long long)k * ldb + n])
                                                    : 0.f;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int e = tid + 256 * i;
      As[TA ? (e / BM) : (e % MBK)][TA ? (e % BM) : (e / MBK)] = ra[i];
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int e = tid + 256 * i;
      Bs[TB ? (e % MBK) : (e / BN)][TB ? (e / MBK) : (e % BN)] = rb[i];
    }
  };
  // NACC interleaved accumulator sets (k-pair s goes to set s % NACC),
  // summed pairwise at the end: a 256-long fp32 fma chain becomes four
  // 64-long ones (the input-gradient and forward GEMMs run K up to 256;
  // the weight-gradient chunks are 32 rows).
  constexpr int NACC = (WG || SPLITQ || TM * TN > 1) ? 1 : 4;  // 128-wide tiles: registers for one set only
  floatx16 acc[NACC][TM][TN];
#pragma unroll
  for (int q = 0; q < NACC; ++q)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[q][i][j] = floatx16{0};
  // bias-gradient column sums (WG, bid.y == 0): column cc, k-quarter cq
  constexpr int CQ = 256 / BN, CK = MBK / CQ;
  const int cc = tid % BN, cq = tid / BN;
  float csum = 0.f;
  const bool do_cs = WG && bid.y == 0;
  const int r = lane & 31, h = lane >> 5;
  if (kbeg < kend) load(kbeg);
  for (int k0 = kbeg; k0 < kend; k0 += MBK) {
    store();
    __syncthreads();
    if (k0 + MBK < kend) load(k0 + MBK);
#pragma unroll
    for (int kb = 0; kb < MBK; kb += 2) {
      float a[TM], b[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) a[i] = As[kb + h][wm0 + 32 * i + r];
#pragma unroll
      for (int j = 0; j < TN; ++j) b[j] = Bs[kb + h][wn0 + 32 * j + r];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[(kb / 2) % NACC][i][j] =
              __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[(kb / 2) % NACC][i][j], 0, 0, 0);
    }
    if (do_cs) {
#pragma unroll
      for (int kk = 0; kk < CK; ++kk) csum += Bs[cq * CK + kk][cc];
    }
    __syncthreads();
  }
  if constexpr (NACC > 1) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
        acc[0][i][j] = NACC == 4 ? (acc[0][i][j] + acc[1][i][j]) + (acc[2][i][j] + acc[3][i][j])
                                 : acc[0][i][j] + acc[1][i][j];
  }
  if (SPLITQ) {
    float* P = C + (long long)bid.z * M * N;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int m = m0 + wm0 + (q & 3) + 8 * (q >> 2) + 4 * h, n = n0 + wn0 + r;
      if (m < M && n < N) P[(long long)m * N + n] = acc[0][0][0][q];
    }
    return;
  }
  if (WG) {
    float* P = C + (long long)bid.z * (M + 1) * N;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int m = m0 + wm0 + 32 * i + (q & 3) + 8 * (q >> 2) + 4 * h, n = n0 + wn0 + 32 * j + r;
          if (m < M && n < N) P[(long long)m * N + n] = acc[0][i][j][q];
        }
    if (do_cs) {
      float* red = &As[0][0];  // free after the loop's last barrier
      red[cq * BN + cc] = csum;
      __syncthreads();
      if (cq == 0 && n0 + cc < N) {
        float v = red[cc];
        for (int q = 1; q < CQ; ++q) v = v + red[q * BN + cc];
        P[(long long)M * N + n0 + cc] = v;
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int m = m0 + wm0 + 32 * i + (q & 3) + 8 * (q >> 2) + 4 * h, n = n0 + wn0 + 32 * j + r;
        if (m < M && n < N)
          gemm_epilogue(acc[0][i][j][q], n, (long long)m * ldc + n, C, epi, bias, H, Z, SW ? ZF_ACT_SWISH : act);
      }
}


template <int BM, int BN, bool TA, bool TB, bool WG, bool SPLITQ = false, bool SW = false>
__global__ __launch_bounds__(256) void mgemm_kernel(int M, int N, int K, const float* __restrict__ A, int lda,
                                                    const float* __restrict__ B, int ldb, float* __restrict__ C,
                                                    int ldc, int epi, const float* __restrict__ bias,
                                                    float* __restrict__ H, const float* __restrict__ Z, int KC,
                                                    int act) {
  mgemm_body<BM, BN, TA, TB, WG, SPLITQ, SW>(uint3{blockIdx.x, blockIdx.y, blockIdx.z}, M, N, K, A, lda, B, ldb, C,
                                             ldc, epi, bias, H, Z, KC, act);
}

__global__ void gemm_combine_kernel(int M, int N, const float* __restrict__ P, float* __restrict__ C, int ldc,
                                    int epi, const float* __restrict__ bias, float* __restrict__ H,
                                    const float* __restrict__ Z, int act) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long MN = (long long)M * N;
  if (i >= MN) return;
  const int m = (int)(i / N), n = (int)(i - (long long)m * N);
  const float v = (P[i] + P[MN + i]) + (P[2 * MN + i] + P[3 * MN + i]);
  gemm_epilogue(v, n, (long long)m * ldc + n, C, epi, bias, H, Z, act);
}

// C = A . B for K <= 8 (the first Dense of a coupling: K = dc + C inputs),
// one thread per output, with the arithmetic of the 64 x 64 interleaved
// MFMA kernel: k-pair p into set p mod 4 as fma(a1, b1, fma(a0, b0, s)) (the
// f32 MFMA's k-ordered fma chain), the tile's all-zero pairs as s + 0 (they
// only turn -0 into +0), then (s0 + s1) + (s2 + s3) and the same epilogue.
// The MFMA kernel would run 32 blocks of one mostly empty k-tile.
__global__ void gemm_small_k_kernel(int M, int N, int K, const float* __restrict__ A, int lda,
                                    const float* __restrict__ B, int ldb, float* __restrict__ C, int ldc, int epi,
                                    const float* __restrict__ bias, float* __restrict__ H,
                                    const float* __restrict__ Z, int act) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)M * N) return;
  const int m = (int)(i / N), n = (int)(i - (long long)m * N);
  float sq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int k = 2 * p;
    if (k < K) {
      const float a0 = A[(long long)m * lda + k], b0 = B[(long long)k * ldb + n];
      const float a1 = k + 1 < K ? A[(long long)m * lda + k + 1] : 0.f;
      const float b1 = k + 1 < K ? B[(long long)(k + 1) * ldb + n] : 0.f;
      sq[p] = __builtin_fmaf(a1, b1, __builtin_fmaf(a0, b0, sq[p]));
    }
  }
  const float v = (__fadd_rn(sq[0], 0.f) + __fadd_rn(sq[1], 0.f)) + (__fadd_rn(sq[2], 0.f) + __fadd_rn(sq[3], 0.f));
  gemm_epilogue(v, n, (long long)m * ldc + n, C, epi, bias, H, Z, act);
}

// gemm_small_k_kernel with four consecutive outputs of kSk4Rows rows per
// thread (N % 4 == 0, 16-B aligned C / H rows): the same fma order per
// output (the same bits), the B columns and bias read once for all rows,
// and one dwordx4 store per array and row.  Grid (ceil(N / 256),
// ceil(M / (4 kSk4Rows))), block (64, 4): no per-thread division.
constexpr int kSk4Rows = 8;
__global__ __launch_bounds__(256) void gemm_small_k4_kernel(int M, int N, int K, const float* __restrict__ A, int lda,
                                     const float* __restrict__ B, int ldb, float* __restrict__ C, int ldc, int epi,
                                     const float* __restrict__ bias, float* __restrict__ H, int act,
                                     unsigned* __restrict__ rmax) {
  const int m0 = (blockIdx.y * 4 + threadIdx.y) * kSk4Rows;
  const int n = 4 * (blockIdx.x * 64 + threadIdx.x);
  if (m0 >= M) return;  // uniform per wave (a wave is one threadIdx.y)
  const bool nok = n < N;
  if (!nok && !rmax) return;
  float b[8][4], bs[4];
#pragma unroll
  for (int k = 0; k < 8; ++k)
#pragma unroll
    for (int t = 0; t < 4; ++t) b[k][t] = nok && k < K ? B[(long long)k * ldb + n + t] : 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t) bs[t] = nok && epi == kEpiBias ? bias[n + t] : 0.f;
  for (int r = 0; r < kSk4Rows; ++r) {
    const int m = m0 + r;
    if (m >= M) break;
    // (a lane past the last column, kept for the row max, multiplies zeros and stores nothing)
    float a[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = k < K ? A[(long long)m * lda + k] : 0.f;
    float out[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      float sq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int k = 2 * p;
        if (k < K) sq[p] = __builtin_fmaf(a[k + 1], b[k + 1][t], __builtin_fmaf(a[k], b[k][t], sq[p]));
      }
      float v = (__fadd_rn(sq[0], 0.f) + __fadd_rn(sq[1], 0.f)) + (__fadd_rn(sq[2], 0.f) + __fadd_rn(sq[3], 0.f));
      if (epi == kEpiBias) v = v + bs[t];
      out[t] = v;
    }
    const long long o = (long long)m * ldc + n;
    float mx = 0.f;
    if (epi == kEpiBias && H) {
      float y[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) y[t] = act == ZF_ACT_SWISH ? out[t] * sigmoidf(out[t]) : act_other(act, out[t]);
      if (nok) *reinterpret_cast<float4*>(H + o) = float4{y[0], y[1], y[2], y[3]};
      if (rmax && nok) mx = fmaxf(fmaxf(fabsf(y[0]), fabsf(y[1])), fmaxf(fabsf(y[2]), fabsf(y[3])));
    } else if (rmax && nok) {
      mx = fmaxf(fmaxf(fabsf(out[0]), fabsf(out[1])), fmaxf(fabsf(out[2]), fabsf(out[3])));
    }
    if (C && nok) *reinterpret_cast<float4*>(C + o) = float4{out[0], out[1], out[2], out[3]};
    if (rmax) {
      // max |row piece| over the wave's 256 columns by DPP (within each
      // 16-lane row, then row_bcast:15 / row_bcast:31 into lane 63: VALU
      // only, no LDS permutes), one atomic per row and wave
#define ZF_DMAX(CTRL, ROWS) \
  mx = fmaxf(mx, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(mx), __float_as_int(mx), CTRL, ROWS, 0xF, false)))
      ZF_DMAX(0xB1, 0xF);   // quad_perm [1, 0, 3, 2]
      ZF_DMAX(0x4E, 0xF);   // quad_perm [2, 3, 0, 1]
      ZF_DMAX(0x141, 0xF);  // row_half_mirror
      ZF_DMAX(0x140, 0xF);  // row_mirror: every lane has its 16-lane row's max
      ZF_DMAX(0x142, 0xA);  // row_bcast:15 into rows 1 and 3
      ZF_DMAX(0x143, 0xC);  // row_bcast:31 into rows 2 and 3: lane 63 has the wave's max
#undef ZF_DMAX
      if (threadIdx.x == 63) atomicMax(rmax + m, __float_as_uint(mx));
    }
  }
}

// ---- Large-batch GEMMs on bf16x3 split MFMA ----------------------------------
// C = A . op(B) (A row-major [M][K]; B row-major [K][N], or [N][K] when TB)
// with every fp32 operand split into three RNE bf16 terms (x = hi + mid + lo)
// and six v_mfma_f32_32x32x16_bf16 products per k-step, small terms first —
// an fp32 dot product to ~1e-7 relative (the inference kernels' bf16x3
// scheme, zf_flow_x3_kernel.h), at 419 TFLOP/s fp32-equivalent peak against
// the fp32 MFMA's 157.  Block tile 128 x 128 x 32, 4 waves in 2 x 2, each
// 64 x 64 as 2 x 2 MFMA tiles.  The split is done once per element, when a
// k-tile is stored to LDS: LDS holds three bf16 planes of A ([m][k]) and of
// B ([n][k]), rows of 32 k padded to 80 B (the 16 rows of a ds_read_b128
// lane group land on 16 distinct 4-bank slots), so the inner loop is
// fragment reads and MFMAs only.  The next k-tile's global loads are in
// flight in registers while the current one is multiplied; 60 KiB of LDS ->
// 2 blocks per CU.  K % 8 == 0 (a ragged last k-tile is zero-filled).
// Epilogue: when N and the output rows allow it (WIDE), B is the MFMA's
// first operand, so a lane holds one output row's 4 consecutive columns per
// register group (same products, same sums, same bits); the tile goes
// through LDS and leaves as row-contiguous dwordx4 stores, whole 128-B lines.
// The MFMA layout's 64 dword stores per lane were store-issue-bound: cfg5's
// hidden layer 111 us with them, 70 us with dwordx4 row pieces
// (tests/hip/gemm_probe.hip).  Same epilogues as mgemm_kernel.  Used when
// the GLOBAL batch gives >= 512 such blocks; ZF_TRAIN_X3=0 keeps the fp32
// kernel.
typedef __bf16 tbf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 tbf16x2 __attribute__((ext_vector_type(2)));
typedef float tfloatx2 __attribute__((ext_vector_type(2)));
constexpr int kX3Plane = 128 * kX3RS;           // bf16 per plane

// three RNE bf16 terms of 8 fp32 values, stored to the three planes at p
__device__ __forceinline__ void split3_store(const float (&x)[8], __bf16* p) {
  tbf16x8 h, m, l;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const tfloatx2 v = {x[2 * i], x[2 * i + 1]};
    const tbf16x2 vh = __builtin_convertvector(v, tbf16x2);
    const tfloatx2 r = v - __builtin_convertvector(vh, tfloatx2);
    const tbf16x2 vm = __builtin_convertvector(r, tbf16x2);
    const tfloatx2 r2 = r - __builtin_convertvector(vm, tfloatx2);
    const tbf16x2 vl = __builtin_convertvector(r2, tbf16x2);
    h[2 * i] = vh[0]; h[2 * i + 1] = vh[1];
    m[2 * i] = vm[0]; m[2 * i + 1] = vm[1];
    l[2 * i] = vl[0]; l[2 * i + 1] = vl[1];
  }
  *reinterpret_cast<tbf16x8*>(p) = h;
  *reinterpret_cast<tbf16x8*>(p + kX3Plane) = m;
  *reinterpret_cast<tbf16x8*>(p + 2 * kX3Plane) = l;
}

template <bool TB, bool WIDE, bool SW>
__global__ __launch_bounds__(256, 2) void gemm_x3_kernel(int M, int N, int K, const float* __restrict__ A, int lda,
                                                      const float* __restrict__ B, int ldb, float* __restrict__ C,
                                                      int ldc, int epi, const float* __restrict__ bias,
                                                      float* __restrict__ H, const float* __restrict__ Z, int act) {
  __shared__ __attribute__((aligned(16))) __bf16 lds[6 * kX3Plane];
  __bf16* const Ap = lds;
  __bf16* const Bp = lds + 3 * kX3Plane;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 64;
  int m0 = 0, n0 = 0;  // the current output tile (the loop below)
  const int r = lane & 31, h = lane >> 5;
  // Register staging of one k-tile: A rows (and B rows when TB) as float4s,
  // B columns as scalars (!TB).  Two sets, filled two k-tiles ahead of the
  // MFMAs that consume them — across output-tile boundaries too, so neither
  // a tile's first k-tile nor any other waits on a full memory latency
  // (one set, one k-tile ahead: Dense 512 x 512 at 0.31 of the MFMA rate).
  struct Stage {
    float4 ra[4], rb[4];
    float rbs[16];
  };
  // Every load is unconditional, from a clamped address, and nothing is
  // computed from a loaded value until its stage is stored: a select right
  // after a load (`ok ? x : 0`) makes the compiler wait for vmcnt(0) there,
  // for the prefetch too.  Rows past M / columns past N read the last one
  // (their outputs are not stored); k past K are zeroed when stored.
  // row-major [rows][K] tiles (A; B when TB): thread -> row e >> 2 (e = tid,
  // tid + 256), 8 consecutive k at 8 (e & 3) as two float4s
  auto load_rows = [&](const float* P, int ld, int r0, int R, int k0, float4 (&v)[4]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = tid + 256 * i, row = min(r0 + (e >> 2), R - 1);
      const float* src = P + (long long)row * ld + min(k0 + 8 * (e & 3), K - 8);
      v[2 * i] = *reinterpret_cast<const float4*>(src);
      v[2 * i + 1] = *reinterpret_cast<const float4*>(src + 4);
    }
  };
  auto store_rows = [&](__bf16* P, const float4 (&v)[4], int k0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = tid + 256 * i;
      const bool kok = k0 + 8 * (e & 3) < K;
      const float4 u = kok ? v[2 * i] : float4{0.f, 0.f, 0.f, 0.f};
      const float4 w = kok ? v[2 * i + 1] : float4{0.f, 0.f, 0.f, 0.f};
      const float x[8] = {u.x, u.y, u.z, u.w, w.x, w.y, w.z, w.w};
      split3_store(x, P + (e >> 2) * kX3RS + 8 * (e & 3));
    }
  };
  // B row-major [K][N] (!TB): thread -> column n0 + (tid & 127), k 16 (tid >> 7) .. +15
  auto load_cols = [&](int tn0, int k0, float (&v)[16]) {
    const int n = min(tn0 + (tid & 127), N - 1);
    const int kb = k0 + 16 * (tid >> 7);
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = B[(long long)min(kb + j, K - 1) * ldb + n];
  };
  auto store_cols = [&](const float (&v)[16], int k0) {
    __bf16* P = Bp + (tid & 127) * kX3RS + 16 * (tid >> 7);
    const int kb = k0 + 16 * (tid >> 7);
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      float x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) x[u] = kb + 8 * g + u < K ? v[8 * g + u] : 0.f;
      split3_store(x, P + 8 * g);
    }
  };
  // persistent blocks: a block takes output tiles blockIdx.x, + gridDim.x,
  // ...; a tile's epilogue stores drain while the next tile's loads and
  // MFMAs run (one launch round of blocks had every block storing at once).
  // The block's k-tiles in order: iteration it = tile ti (the ti-th of this
  // block) x kt k-tiles + k-tile kk.
  const int tiles_n = (N + kX3BN - 1) / kX3BN;
  const int ntiles = tiles_n * ((M + kX3BM - 1) / kX3BM);
  // k-tiles per output tile, rounded up to even (an odd K / 32's extra
  // k-tile is past K: zeroed when stored) so the tile loop below runs them
  // as (S0, S1) pairs and the epilogue is emitted once (three inlined
  // copies of the generic epilogue made the kernel too big for the
  // instruction cache; SW, swish couplings, leaves out the other
  // activations' code)
  const int kt = ((K + kX3BK - 1) / kX3BK + 1) & ~1;
  const int mine = ntiles > (int)blockIdx.x ? (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x : 0;
  const int total = mine * kt;
  auto load = [&](int it, Stage& st) __attribute__((always_inline)) {
    const int ti = it / kt, k0 = (it - ti * kt) * kX3BK;
    const int tile = x3_tile(ti, ntiles);
    const int tm0 = (tile / tiles_n) * kX3BM, tn0 = (tile - (tile / tiles_n) * tiles_n) * kX3BN;
    load_rows(A, lda, tm0, M, k0, st.ra);
    if (TB) load_rows(B, ldb, tn0, N, k0, st.rb);
    else load_cols(tn0, k0, st.rbs);
  };
  if (total == 0) return;
  // Straight-line staging (gemm_h2_kernel, zf_layered.hip): both stages
  // loaded before the loop, two k-steps per iteration with unconditional
  // refills, an odd last k-step after it — a skipped refill on any path
  // leaves the compiler unsure which stage is newest, and it then waits for
  // every load at each stage store (Dense 512 x 512 eval: 1.4x faster).
  Stage S0, S1;
  load(0, S0);
  load(min(1, total - 1), S1);
  floatx16 acc[2][2];
  auto epilogue = [&]() __attribute__((always_inline)) {
    if (WIDE) {
      // through LDS (free after the loop's last barrier), per wave and per
      // 32-row half: ds_write_b128 of each lane's row pieces (row pitch 68
      // floats: conflict-free), then row-contiguous float4s — each store
      // instruction writes 4 rows x 256 B, whole 128-B lines
      float* T = reinterpret_cast<float*>(lds) + wave * (32 * 68);
  #pragma unroll
      for (int i = 0; i < 2; ++i) {
  #pragma unroll
        for (int j = 0; j < 2; ++j)
  #pragma unroll
          for (int g = 0; g < 4; ++g)
            *reinterpret_cast<float4*>(T + r * 68 + 32 * j + 8 * g + 4 * h) =
                float4{acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
        __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the wave's own LDS writes
        __builtin_amdgcn_wave_barrier();
  #pragma unroll
        for (int t = 0; t < 8; ++t) {
          const int row = 4 * t + (lane >> 4), c4 = lane & 15;
          const float4 v = *reinterpret_cast<const float4*>(T + row * 68 + 4 * c4);
          const int m = m0 + wm0 + 32 * i + row, n = n0 + wn0 + 4 * c4;
          if (m < M && n < N) gemm_epilogue4(v, n, (long long)m * ldc + n, C, epi, bias, H, Z, SW ? ZF_ACT_SWISH : act);
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
      }
    } else {
  #pragma unroll
      for (int i = 0; i < 2; ++i)
  #pragma unroll
        for (int j = 0; j < 2; ++j)
  #pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int m = m0 + wm0 + 32 * i + (q & 3) + 8 * (q >> 2) + 4 * h, n = n0 + wn0 + 32 * j + r;
            if (m < M && n < N)
              gemm_epilogue(acc[i][j][q], n, (long long)m * ldc + n, C, epi, bias, H, Z, SW ? ZF_ACT_SWISH : act);
          }
    }
    __syncthreads();  // the next tile's planes overwrite the epilogue's LDS
  };
  // one k-iteration from stage S (refilled with iteration it + 2 once stored)
  auto kstep = [&](int it, int kk, Stage& S) __attribute__((always_inline)) {
    store_rows(Ap, S.ra, kk * kX3BK);
    if (TB) store_rows(Bp, S.rb, kk * kX3BK);
    else store_cols(S.rbs, kk * kX3BK);
    __syncthreads();
    load(min(it + 2, total - 1), S);  // (the last two refills repeat a k-tile, unused)
#pragma unroll
    for (int s = 0; s < kX3BK / 16; ++s) {
      tbf16x8 af[2][3], bf[2][3];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          af[i][t] = *reinterpret_cast<const tbf16x8*>(Ap + t * kX3Plane + (wm0 + 32 * i + r) * kX3RS + 16 * s + 8 * h);
          bf[i][t] = *reinterpret_cast<const tbf16x8*>(Bp + t * kX3Plane + (wn0 + 32 * i + r) * kX3RS + 16 * s + 8 * h);
        }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          // WIDE: B as the MFMA's first operand, so D = C^T: lane = row m and
          // each group of 4 registers = 4 consecutive columns (one dwordx4
          // store; the same products and sums, the same bits)
          auto mf = [&](int ta, int tb, const floatx16& c) {
            return WIDE ? __builtin_amdgcn_mfma_f32_32x32x16_bf16(bf[j][tb], af[i][ta], c, 0, 0, 0)
                        : __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][ta], bf[j][tb], c, 0, 0, 0);
          };
          floatx16 c = mf(1, 1, acc[i][j]);  // (A term, B term): m m, h l, l h, h m, m h, h h
          c = mf(0, 2, c);
          c = mf(2, 0, c);
          c = mf(0, 1, c);
          c = mf(1, 0, c);
          acc[i][j] = mf(0, 0, c);
        }
    }
    __syncthreads();
  };
  int it = 0;
  for (int ti = 0; ti < mine; ++ti) {
    const int tile = x3_tile(ti, ntiles);
    m0 = (tile / tiles_n) * kX3BM;
    n0 = (tile - (tile / tiles_n) * tiles_n) * kX3BN;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = floatx16{0};
    for (int kk = 0; kk < kt; kk += 2, it += 2) {
      kstep(it, kk, S0);
      kstep(it + 1, kk + 1, S1);
    }
    epilogue();
  }
}

// max |H[m][0..N)| as float bits into r[m] (a producer without the fused row max)
__global__ __launch_bounds__(256) void row_absmax_kernel(int M, int N, const float* __restrict__ H, int ldh,
                                                         unsigned* __restrict__ r) {
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (m >= M) return;
  float mx = 0.f;
  for (int n = lane; n < N; n += 64) mx = fmaxf(mx, fabsf(H[(long long)m * ldh + n]));
#pragma unroll
  for (int w = 1; w < 64; w <<= 1) mx = fmaxf(mx, __shfl_xor(mx, w));
  if (lane == 0) r[m] = __float_as_uint(mx);
}

// The swish-only epilogue (SW) whenever no other activation is applied.
inline bool swish_only(int epi, const float* H, int act) {
  return act == ZF_ACT_SWISH || epi == kEpiNone || (epi == kEpiBias && !H);
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int T>
void gemm_launch(bool tb, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                 hipStream_t st, int epi, const float* bias, float* H, const float* Z, int act) {
  const dim3 grid((N + T - 1) / T, (M + T - 1) / T);
  const bool sw = swish_only(epi, H, act);
#define ZF_MG_LAUNCH(TB_, SW_)                                                                                \
  hipLaunchKernelGGL((mgemm_kernel<T, T, false, TB_, false, false, SW_>), grid, dim3(256), 0, st, M, N, K, A, lda, \
                     B, ldb, C, ldc, epi, bias, H, Z, 0, act)
  if (!tb) {
    if (sw) ZF_MG_LAUNCH(false, true);
    else ZF_MG_LAUNCH(false, false);
  } else {
    if (sw) ZF_MG_LAUNCH(true, true);
    else ZF_MG_LAUNCH(true, false);
  }
#undef ZF_MG_LAUNCH
}

// C = A . op(B) with A row-major [M][K]; 128 x 128 tiles when they give at
// least 512 blocks over the GLOBAL batch's Mg rows, 64 x 64 otherwise.  The
// two tiles accumulate differently (one chain vs four interleaved), so the
// choice follows the global batch: every data-parallel shard then runs the
// kernel, and gets the bits, of the one-device step.  64 x 64 tiles that
// would leave most CUs idle (< 256 blocks, K >= 64) run as the four split
// sets + combine (SPLITQ; same bits) when a workspace of 4 M N floats is
// given (`split`, the trainer's split-K buffer), and K <= 8 as one thread
// per output (gemm_small_k_kernel; same bits); ZF_TRAIN_SPLITQ=0: neither.
int gemm(bool tb, long long Mg, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C,
         int ldc, hipStream_t st, int epi = kEpiNone, const float* bias = nullptr, float* H = nullptr,
         const float* Z = nullptr, int act = ZF_ACT_SWISH, float* split = nullptr, long long split_cap = 0,
         unsigned* rmax = nullptr, bool* rmax_done = nullptr) {
  if (M <= 0 || N <= 0) return ZF_OK;
  const long long big = (long long)((N + 127) / 128) * ((Mg + 127) / 128);
  const long long tiles64 = (long long)((N + 63) / 64) * ((M + 63) / 64);
  static const bool x3_ok = [] {
    const char* e = std::getenv("ZF_TRAIN_X3");
    return !(e && e[0] == '0');
  }();
  const bool a_ok = lda % 4 == 0 && (reinterpret_cast<uintptr_t>(A) & 15) == 0;
  const bool b_ok = !tb || (ldb % 4 == 0 && (reinterpret_cast<uintptr_t>(B) & 15) == 0);
  if (big >= 512 && !tb && K <= 8) {
    // the first Dense (K = dc + C <= 8) at large batches too: one thread per
    // output is bound by its Z / H stores, the MFMA tiles would multiply a
    // 32-deep k-tile of zeros (the choice follows the global batch, as below;
    // not a split-set form, so ZF_TRAIN_SPLITQ=0 keeps it)
    const long long MN = (long long)M * N;
    if (N % 4 == 0 && ldc % 4 == 0 && al16(C) && al16(H) && (epi == kEpiBias || epi == kEpiNone)) {
      hipLaunchKernelGGL(gemm_small_k4_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)((M + 4 * kSk4Rows - 1) / (4 * kSk4Rows))),
                         dim3(64, 4), 0, st, M, N, K, A, lda, B, ldb, C, ldc, epi, bias, H, act, rmax);
      ZF_CHECK_LAUNCH("gemm_small_k4_kernel");
      if (rmax_done) *rmax_done = rmax != nullptr;
      return ZF_OK;
    }
    hipLaunchKernelGGL(gemm_small_k_kernel, dim3((unsigned)((MN + 255) / 256)), dim3(256), 0, st, M, N, K, A, lda, B,
                       ldb, C, ldc, epi, bias, H, Z, act);
    ZF_CHECK_LAUNCH("gemm_small_k_kernel");
    return ZF_OK;
  }
  if (big >= 512 && x3_ok && K % 8 == 0 && a_ok && b_ok) {
    // two resident blocks per CU (60 KiB of LDS each), persistent over the tiles
    const long long ntiles = (long long)((N + kX3BN - 1) / kX3BN) * ((M + kX3BM - 1) / kX3BM);
    int dev = 0, ncu = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    const dim3 grid((unsigned)std::min<long long>(ntiles, 2ll * ncu));
    const bool wide = N % 4 == 0 && ldc % 4 == 0 && al16(C) && (!H || al16(H)) && (!Z || al16(Z));
    const bool sw = swish_only(epi, H, act);
#define ZF_X3_LAUNCH(TB_, W_, S_)                                                                                    \
  hipLaunchKernelGGL((gemm_x3_kernel<TB_, W_, S_>), grid, dim3(256), 0, st, M, N, K, A, lda, B, ldb, C, ldc, epi, \
                     bias, H, Z, act)
#define ZF_X3_LAUNCH_SW(TB_, W_) \
  if (sw) ZF_X3_LAUNCH(TB_, W_, true); else ZF_X3_LAUNCH(TB_, W_, false)
    if (tb) {
      if (wide) ZF_X3_LAUNCH_SW(true, true);
      else ZF_X3_LAUNCH_SW(true, false);
    } else {
      if (wide) ZF_X3_LAUNCH_SW(false, true);
      else ZF_X3_LAUNCH_SW(false, false);
    }
#undef ZF_X3_LAUNCH_SW
#undef ZF_X3_LAUNCH
    ZF_CHECK_LAUNCH("gemm_x3_kernel");
    return ZF_OK;
  }
  if (big >= 512) {
    gemm_launch<128>(tb, M, N, K, A, lda, B, ldb, C, ldc, st, epi, bias, H, Z, act);
  } else if (split != nullptr && !tb && K <= 8) {
    const long long MN = (long long)M * N;
    hipLaunchKernelGGL(gemm_small_k_kernel, dim3((unsigned)((MN + 255) / 256)), dim3(256), 0, st, M, N, K, A, lda, B,
                       ldb, C, ldc, epi, bias, H, Z, act);
  } else if (split != nullptr && tiles64 < 256 && K >= 64 && 4ll * M * N <= split_cap) {
    const dim3 grid((N + 63) / 64, (M + 63) / 64, 4);
    if (!tb)
      hipLaunchKernelGGL((mgemm_kernel<64, 64, false, false, false, true>), grid, dim3(256), 0, st, M, N, K, A, lda, B,
                         ldb, split, N, kEpiNone, nullptr, nullptr, nullptr, 0, act);
    else
      hipLaunchKernelGGL((mgemm_kernel<64, 64, false, true, false, true>), grid, dim3(256), 0, st, M, N, K, A, lda, B,
                         ldb, split, N, kEpiNone, nullptr, nullptr, nullptr, 0, act);
    ZF_CHECK_LAUNCH("mgemm_kernel<splitq>");
    const long long MN = (long long)M * N;
    hipLaunchKernelGGL(gemm_combine_kernel, dim3((unsigned)((MN + 255) / 256)), dim3(256), 0, st, M, N, split, C, ldc,
                       epi, bias, H, Z, act);
  } else {
    gemm_launch<64>(tb, M, N, K, A, lda, B, ldb, C, ldc, st, epi, bias, H, Z, act);
  }
  ZF_CHECK_LAUNCH("mgemm_kernel");
  return ZF_OK;
}

}  // namespace
}  // namespace zf
