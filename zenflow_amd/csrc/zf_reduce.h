// Batch reductions of the trainer: row leaves summed in row order and one
// fixed pairwise fp64 tree over them (Leaves / leaves_for, tree_n, lds_tree),
// the tree kernels, the weight-gradient GEMMs with their deferred queue
// (wgrad*, WgradQueue), the leaf sums and launch_tree_cols.  zenflow_amd/dist.py
// mirrors leaves_for; zf_optim.hip restates the tree for 256 leaves.
#pragma once
#include "zf_gemm.h"

#include <algorithm>
#include <cstdint>

namespace zf {
namespace {

inline unsigned blocks_for(long long n, int t = 256) { return (unsigned)((n + t - 1) / t); }

// a mod m in [0, m): the column of a rotated state (Roll is an index rotation)
__host__ __device__ __forceinline__ int pmodi(int a, int m) {
  int r = a % m;
  return r < 0 ? r + m : r;
}

// Split-K workspace (floats) shared by the batch reductions below.
constexpr int64_t kWsFloats = 32ll << 20;
// The split-set GEMMs' partials (4 M N floats, M N < 256 tiles of 64 x 64).
constexpr int64_t kSplitFloats = 4ll << 20;

// ---- batch reductions: row leaves + one fixed pairwise tree ----------------
// Every sum over the batch rows (weight and bias gradients, BatchNorm sums
// forward and reverse, the loss) is formed the same way: the rows are cut
// into n contiguous leaves of `rows` rows, each leaf is summed in row order,
// and the leaves are combined in fp64 by the pairwise tree
// ((l0 + l1) + (l2 + l3)) + ... (tree_n).  The global leaf count is a power of
// two that depends on the GLOBAL batch size only (leaves_for); under data
// parallelism rank r holds leaves [r n, (r+1) n) of it, reduces that subtree,
// and the ranks' subtree roots are all-gathered and combined by the top of
// the same tree.  So every rank gets the same bits, and R ranks reproduce
// one rank's bits on the same global batch (R a power of two dividing the
// leaf count, shards of B/R rows, B a multiple of the leaf count).
constexpr int kMaxLeaves = 64;        // one tree level (registers)
constexpr int kLeafCap = kMaxLeaves * kMaxLeaves;  // two levels: up to 4096 leaves

inline int pow2floor(long long v) {
  int p = 1;
  while ((long long)p * 2 <= v && p < (1 << 30)) p *= 2;
  return p;
}

struct Leaves {
  int n;     // this rank's leaves (a power of two)
  int rows;  // rows per leaf (the last one may be short or empty)
};

// ~32 rows per leaf, at most `cap` (a power of two) leaves in the whole batch.
inline Leaves leaves_for(long long B_loc, long long Bg, int world, int cap) {
  const long long want = std::max<long long>(1, std::min<long long>(Bg / 32, cap));
  Leaves l;
  l.n = std::max(1, pow2floor(want / std::max(1, world)));
  l.rows = (int)((B_loc + l.n - 1) / l.n);
  return l;
}

// Pairwise tree over p[0], p[stride], ..., p[(n-1) stride] (n <= NMAX <= 64)
// in fp64: level s adds element i + s into i for i a multiple of 2s (the
// perfect tree for a power of two; a shorter tail just joins later).  NMAX
// only sizes the register array: every NMAX >= n gives the same bits.
template <int NMAX, typename TI>
__device__ __forceinline__ double tree_n(const TI* __restrict__ p, long long stride, int n) {
  double v[NMAX];
#pragma unroll
  for (int i = 0; i < NMAX; ++i) v[i] = i < n ? (double)p[i * stride] : 0.0;
#pragma unroll
  for (int s = 1; s < NMAX; s *= 2)
#pragma unroll
    for (int i = 0; i < NMAX; i += 2 * s)
      if (i + s < n) v[i] = v[i] + v[i + s];
  return v[0];
}

// The same tree in place over LDS columns (leaf i of column k at
// p[i * stride + k]), all threads of the block taking part, one barrier per
// level: the same pairings and operand order as tree_n.  Result in p[k].
__device__ __forceinline__ void lds_tree(double* p, int n, int ncols, int stride) {
  for (int s = 1; s < n; s *= 2) {
    const int pairs = (n + 2 * s - 1) / (2 * s);
    for (int t = threadIdx.x; t < pairs * ncols; t += blockDim.x) {
      const int j = t / ncols, k = t - j * ncols, i = 2 * s * j;
      if (i + s < n) p[i * stride + k] = p[i * stride + k] + p[(i + s) * stride + k];
    }
    __syncthreads();
  }
}

// Two such trees (same shapes) level by level under one barrier per level:
// each tree's pairwise sums are unchanged.
__device__ __forceinline__ void lds_tree2(double* p, double* q, int n, int ncols, int stride) {
  for (int s = 1; s < n; s *= 2) {
    const int pairs = (n + 2 * s - 1) / (2 * s);
    for (int t = threadIdx.x; t < pairs * ncols; t += blockDim.x) {
      const int j = t / ncols, k = t - j * ncols, i = 2 * s * j;
      if (i + s < n) {
        p[i * stride + k] = p[i * stride + k] + p[(i + s) * stride + k];
        q[i * stride + k] = q[i * stride + k] + q[(i + s) * stride + k];
      }
    }
    __syncthreads();
  }
}

// Launch KERNEL<..., NMAX> with the smallest register tree that holds n leaves.
#define ZF_NMAX_DISPATCH(n, LAUNCH) \
  do {                              \
    if ((n) <= 8) LAUNCH(8);        \
    else if ((n) <= 16) LAUNCH(16); \
    else if ((n) <= 32) LAUNCH(32); \
    else LAUNCH(64);                \
  } while (0)

// out[k] = tree over n leaves of part[leaf * N + k]
template <typename TI, int NMAX>
__global__ void tree_cols_kernel(const TI* __restrict__ part, int n, long long N, double* __restrict__ out) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < N) out[k] = tree_n<NMAX>(part + k, N, n);
}

// First level of a two-level tree: out[g * N + k] = tree over the 64 leaves
// [64 g, 64 g + 64) of part (a perfect subtree of the power-of-two leaf tree,
// so the second level over the group roots completes the same tree).
template <typename TI>
__global__ void tree_groups_kernel(const TI* __restrict__ part, int groups, long long N, double* __restrict__ out) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)groups * N) return;
  const long long g = t / N, k = t - g * N;
  out[t] = tree_n<kMaxLeaves>(part + g * kMaxLeaves * N + k, N, kMaxLeaves);
}

// same, then the final fp32 rounding (the gradient handed to the optimiser)
template <int NMAX>
__global__ void tree_cols_cast_kernel(const double* __restrict__ part, int n, long long N, float* __restrict__ out) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < N) out[k] = (float)tree_n<NMAX>(part + k, N, n);
}

// dW/db from the split-K partials part[leaf][M+1][N] (fp32 leaf GEMMs, or
// their fp64 group roots), combined by the leaf tree into the fp64 gradient
// accumulator.
// dW / db from the n (a power of two) leaf partials of each element: the
// four waves of a block each reduce a perfect subtree of n / 4 consecutive
// leaves for 64 elements (n < 4: one wave per leaf), joined as the top two
// levels of the same tree — four times the waves of a thread-per-element tree
// for the same bits.
template <typename TI, int NMAX>
__global__ __launch_bounds__(256) void wgrad_tree(int M, int N, int n, const TI* __restrict__ part,
                                                  double* __restrict__ dW, double* __restrict__ db) {
  __shared__ double r[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int P = n < 4 ? n : 4, m = n / P;
  const long long idx = (long long)blockIdx.x * 64 + lane;
  const long long MN1 = (long long)(M + 1) * N;
  if (w < P && idx < MN1) r[w][lane] = tree_n<NMAX>(part + (long long)w * m * MN1 + idx, MN1, m);
  __syncthreads();
  if (w != 0 || idx >= MN1) return;
  double v = r[0][lane];
  if (P == 2) v = v + r[1][lane];
  else if (P == 4) v = (v + r[1][lane]) + (r[2][lane] + r[3][lane]);
  if (idx < (long long)M * N) dW[idx] = v;
  else db[idx - (long long)M * N] = v;
}

// dW[M,N] = A^T . G and db[N] = colsum(G), A row-major [B][M] (layer input),
// G row-major [B][N] (gradient of the layer output): one split-K block per
// leaf (rows [z lv.rows, (z+1) lv.rows)), then wgrad_tree.
int wgrad(int M, int N, int B, const Leaves& lv, const float* A, const float* G, double* dW, double* db, float* ws,
          double* ws2, hipStream_t st) {
  constexpr int T = 64;
  const int64_t MN1 = (int64_t)(M + 1) * N;
  if ((int64_t)lv.n * MN1 > kWsFloats) return enotsup("training: weight-gradient workspace");
  hipLaunchKernelGGL((mgemm_kernel<T, T, true, false, true>), dim3((N + T - 1) / T, (M + T - 1) / T, lv.n),
                     dim3(256), 0, st, M, N, B, A, M, G, N, ws, N, kEpiNone, nullptr, nullptr, nullptr, lv.rows,
                     (int)ZF_ACT_SWISH);
  ZF_CHECK_LAUNCH("mgemm_kernel<wgrad>");
  if (lv.n <= kMaxLeaves) {
#define ZF_L(NM) hipLaunchKernelGGL((wgrad_tree<float, NM>), dim3(blocks_for(MN1, 64)), dim3(256), 0, st, M, N, lv.n, ws, dW, db)
    ZF_NMAX_DISPATCH(lv.n < 4 ? 1 : lv.n / 4, ZF_L);
#undef ZF_L
  } else {  // two levels: groups of 64 leaves, then their roots
    const int groups = lv.n / kMaxLeaves;
    hipLaunchKernelGGL(tree_groups_kernel<float>, dim3(blocks_for((int64_t)groups * MN1)), dim3(256), 0, st, ws,
                       groups, MN1, ws2);
    ZF_CHECK_LAUNCH("tree_groups_kernel");
#define ZF_L(NM) hipLaunchKernelGGL((wgrad_tree<double, NM>), dim3(blocks_for(MN1, 64)), dim3(256), 0, st, M, N, groups, ws2, dW, db)
    ZF_NMAX_DISPATCH(groups < 4 ? 1 : groups / 4, ZF_L);
#undef ZF_L
  }
  ZF_CHECK_LAUNCH("wgrad_tree");
  return ZF_OK;
}

// Weight-gradient trees of several layers in one launch: the backward pass
// writes each layer's leaf partials to its own slice of the split-K
// workspace and the trees of all of them run at the end (or when the
// workspace or the item list is full) — one launch instead of one per layer,
// the same per-element trees (wgrad_tree's), so the same bits.
constexpr int kTreeItems = 24;
struct TreeItem {
  const float* part;
  double* dW;
  double* db;
  int M, N, n, blocks;  // blocks of 64 elements
};
struct TreeBatch {
  int count;
  TreeItem it[kTreeItems];
};

template <int NMAX>
__global__ __launch_bounds__(256) void wgrad_tree_batch(TreeBatch tb) {
  __shared__ double r[4][64];
  int b = blockIdx.x, i = 0;
  while (i + 1 < tb.count && b >= tb.it[i].blocks) b -= tb.it[i++].blocks;
  const TreeItem& t = tb.it[i];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int P = t.n < 4 ? t.n : 4, m = t.n / P;
  const long long idx = (long long)b * 64 + lane;
  const long long MN1 = (long long)(t.M + 1) * t.N;
  if (w < P && idx < MN1) r[w][lane] = tree_n<NMAX>(t.part + (long long)w * m * MN1 + idx, MN1, m);
  __syncthreads();
  if (w != 0 || idx >= MN1) return;
  double v = r[0][lane];
  if (P == 2) v = v + r[1][lane];
  else if (P == 4) v = (v + r[1][lane]) + (r[2][lane] + r[3][lane]);
  if (idx < (long long)t.M * t.N) t.dW[idx] = v;
  else t.db[idx - (long long)t.M * t.N] = v;
}

// Weight-gradient GEMMs deferred into one launch: each problem is the
// mgemm_kernel<64, 64, TA, !TB, WG> grid it would have launched on its own
// (the same blocks, the same bits), laid end to end.
struct WgGemm {
  const float *A, *G;
  float* part;
  int M, N, B, rows, tx, ty, block0;
};
constexpr int kWgGroup = 8;
struct WgGroup {
  int count;
  WgGemm g[kWgGroup];
};

__global__ __launch_bounds__(256) void wgrad_group_kernel(WgGroup grp) {
  int i = 0;
  while (i + 1 < grp.count && (int)blockIdx.x >= grp.g[i + 1].block0) ++i;
  const WgGemm& g = grp.g[i];
  int r = (int)blockIdx.x - g.block0;
  const unsigned bx = r % g.tx;
  r /= g.tx;
  const unsigned by = r % g.ty, bz = r / g.ty;
  mgemm_body<64, 64, true, false, true, false>(uint3{bx, by, bz}, g.M, g.N, g.B, g.A, g.M, g.G, g.N, g.part, g.N,
                                               kEpiNone, nullptr, nullptr, nullptr, g.rows, (int)ZF_ACT_SWISH);
}

struct WgradQueue {
  TreeBatch tb;
  WgGroup gq;        // GEMMs not launched yet
  int gblocks = 0;   // their blocks
  int64_t used = 0;  // workspace floats holding pending partials
  int nmax = 1;
};

int wgrad_launch_gemms(WgradQueue& q, hipStream_t st) {
  if (q.gq.count == 0) return ZF_OK;
  hipLaunchKernelGGL(wgrad_group_kernel, dim3(q.gblocks), dim3(256), 0, st, q.gq);
  ZF_CHECK_LAUNCH("wgrad_group_kernel");
  q.gq.count = 0;
  q.gblocks = 0;
  return ZF_OK;
}

// Launch the deferred GEMMs before `p` (a buffer one of them reads) is
// overwritten.
int wgrad_before_write(WgradQueue& q, const float* p, hipStream_t st) {
  for (int i = 0; i < q.gq.count; ++i)
    if (q.gq.g[i].A == p || q.gq.g[i].G == p) return wgrad_launch_gemms(q, st);
  return ZF_OK;
}

int wgrad_flush(WgradQueue& q, hipStream_t st) {
  int rc = wgrad_launch_gemms(q, st);
  if (rc) return rc;
  if (q.tb.count == 0) return ZF_OK;
  int blocks = 0;
  for (int i = 0; i < q.tb.count; ++i) blocks += q.tb.it[i].blocks;
  const int nm = q.nmax < 4 ? 1 : q.nmax / 4;
#define ZF_L(NM) hipLaunchKernelGGL((wgrad_tree_batch<NM>), dim3(blocks), dim3(256), 0, st, q.tb)
  ZF_NMAX_DISPATCH(nm, ZF_L);
#undef ZF_L
  ZF_CHECK_LAUNCH("wgrad_tree_batch");
  q.tb.count = 0;
  q.used = 0;
  q.nmax = 1;
  return ZF_OK;
}

// wgrad with the tree deferred into `q` (one level of leaves: n <= 64);
// more leaves run wgrad's two-level form at once, after the queue.
int wgrad_deferred(WgradQueue& q, int M, int N, int B, const Leaves& lv, const float* A, const float* G, double* dW,
                   double* db, float* ws, double* ws2, hipStream_t st) {
  const int64_t MN1 = (int64_t)(M + 1) * N, need = (int64_t)lv.n * MN1;
  int rc;
  if (lv.n > kMaxLeaves) {
    if ((rc = wgrad_flush(q, st))) return rc;
    return wgrad(M, N, B, lv, A, G, dW, db, ws, ws2, st);
  }
  if (need > kWsFloats) return enotsup("training: weight-gradient workspace");
  if (q.used + need > kWsFloats || q.tb.count == kTreeItems)
    if ((rc = wgrad_flush(q, st))) return rc;
  float* part = ws + q.used;
  if (q.gq.count == kWgGroup && (rc = wgrad_launch_gemms(q, st))) return rc;
  WgGemm& g = q.gq.g[q.gq.count++];
  g.A = A;
  g.G = G;
  g.part = part;
  g.M = M;
  g.N = N;
  g.B = B;
  g.rows = lv.rows;
  g.tx = (N + 63) / 64;
  g.ty = (M + 63) / 64;
  g.block0 = q.gblocks;
  q.gblocks += g.tx * g.ty * lv.n;
  TreeItem& it = q.tb.it[q.tb.count++];
  it.part = part;
  it.dW = dW;
  it.db = db;
  it.M = M;
  it.N = N;
  it.n = lv.n;
  it.blocks = (int)blocks_for(MN1, 64);
  q.used += need;
  q.nmax = std::max(q.nmax, lv.n);
  return ZF_OK;
}

// Leaf sums of two per-column sums over rows [b0, b1), in row order, fp64:
// s1 = sum x, s2 = sum x * y (y = x: the sum of squares).
constexpr int kLeafInflight = 32;
template <class FX, class FY>
__device__ __forceinline__ void leaf_sums2(FX x_at, FY y_at, int b0, int b1, double& s1, double& s2) {
  double a = 0.0, q = 0.0;
  int b = b0;
  // kLeafInflight rows' loads in flight before their (in-order) sums: the
  // leaf is a chain of dependent adds, its loads are not (the one-block
  // BatchNorm kernels expose every serial round trip: 32 rows, a whole leaf
  // at the default batch, in one)
  constexpr int R = kLeafInflight;
  for (; b + R <= b1; b += R) {
    float xv[R], yv[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
      xv[j] = x_at(b + j);
      yv[j] = y_at(b + j);
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
      a += (double)xv[j];
      q += (double)xv[j] * (double)yv[j];
    }
  }
  for (; b < b1; ++b) {
    const double xv = (double)x_at(b), yv = (double)y_at(b);
    a += xv;
    q += xv * yv;
  }
  s1 = a;
  s2 = q;
}

// One thread per (leaf z, column k): p[z][k] = sum x, p[z][N + k] = sum x*y
// over the leaf's rows of X, Y row-major [B][N] (Y NULL: Y = X).
__global__ void leaf_colsums_kernel(const float* __restrict__ X, const float* __restrict__ Y, int B, int N, int rows,
                                    int n, double* __restrict__ p) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * N) return;
  const int z = t / N, k = t - z * N;
  const int b0 = min(B, z * rows), b1 = min(B, b0 + rows);
  const float* Yp = Y ? Y : X;
  leaf_sums2([&](int b) { return X[(long long)b * N + k]; }, [&](int b) { return Yp[(long long)b * N + k]; }, b0, b1,
             p[(long long)z * 2 * N + k], p[(long long)z * 2 * N + N + k]);
}

// Leaf sums of one column vector (the per-row loss), fp64 in row order.
__global__ void leaf_sum_kernel(const double* __restrict__ x, int B, int rows, int n, double* __restrict__ p) {
  const int z = blockIdx.x * blockDim.x + threadIdx.x;
  if (z >= n) return;
  const int b0 = min(B, z * rows), b1 = min(B, b0 + rows);
  double a = 0.0;
  for (int b = b0; b < b1; ++b) a += x[b];
  p[z] = a;
}

// out[k] = tree over n leaves (a power of two up to kLeafCap, or any n <= 64)
// of part[leaf * N + k]; tmp: (n / 64) * N doubles for the two-level case.
inline int launch_tree_cols(const double* part, int n, long long N, double* out, hipStream_t st,
                            double* tmp = nullptr) {
  if (n > kMaxLeaves) {
    if (!tmp) return einval("tree over %d leaves needs a workspace", n);
    const int groups = n / kMaxLeaves;
    hipLaunchKernelGGL(tree_groups_kernel<double>, dim3(blocks_for((long long)groups * N)), dim3(256), 0, st, part,
                       groups, N, tmp);
    ZF_CHECK_LAUNCH("tree_groups_kernel");
    part = tmp;
    n = groups;
  }
#define ZF_L(NM) hipLaunchKernelGGL((tree_cols_kernel<double, NM>), dim3(blocks_for(N)), dim3(256), 0, st, part, n, N, out)
  ZF_NMAX_DISPATCH(n, ZF_L);
#undef ZF_L
  ZF_CHECK_LAUNCH("tree_cols_kernel");
  return ZF_OK;
}

}  // namespace
}  // namespace zf
